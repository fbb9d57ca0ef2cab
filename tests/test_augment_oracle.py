"""The augmentation without a GPU: the numpy oracle against closed forms, `draw` (reproducible per sample, valid weight sets, gate
frequencies), the library of its own (group, header, exports, signatures, source hash, kernel resources), the refusals of the C entry point
and of the wrapper on host memory, and the two helpers against the reference's formulas."""
import ctypes
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import augment_cases as cases, augment_oracle as oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _off(B=1):
    return np.zeros((B, 64), dtype=np.int32), np.tile(np.arange(256, dtype=np.uint8), (B, 3, 1))


# ---- the oracle against closed forms


def test_all_stages_off_is_the_identity():
    crops, bg, msk, lut = cases.make_inputs(9, 13, 2, 1)
    params, _ = _off(2)
    out, info = oracle.augment(crops, params, lut, msk, bg, seed=5)
    assert np.array_equal(out, crops) and not info.any()


def test_blend_ends_and_ties():
    fg = np.full((3, 1, 6), 200, np.uint8)
    bg = np.array([10, 11, 12, 13, 10, 10], np.uint8)[None, None].repeat(3, 0)
    msk = np.array([[0.0, 1.0, 0.5, 0.5, np.nan, 2.0]], np.float32)
    got = oracle.blend(fg, bg, msk)[0, 0]
    # k = 0: the background; k = 1024: the crop; (200 + 12) / 2 = 106 exactly; (200 + 13) / 2 = 106.5 -> 106 (even); NaN -> k = 0; 2 -> k = 1024
    assert got.tolist() == [10, 200, 106, 106, 10, 200]
    assert oracle.blend(np.full((3, 1, 1), 201, np.uint8), np.full((3, 1, 1), 14, np.uint8), np.array([[0.5]], np.float32))[0, 0, 0] == 108  # 107.5 -> 108
    params, lut = _off(1)
    params[0, 0] = 1
    crops = np.full((1, 3, 8, 8), 7, np.uint8)
    back = np.full((1, 3, 8, 8), 99, np.uint8)
    assert (oracle.augment(crops, params, lut, np.zeros((1, 8, 8), np.float32), back)[0] == 99).all()
    assert (oracle.augment(crops, params, lut, np.ones((1, 8, 8), np.float32), back)[0] == 7).all()


@pytest.mark.parametrize("bit,lo", [(cases.FILTER_A, 6), (cases.FILTER_B, 31)])
def test_delta_image_returns_the_mirrored_weights(bit, lo):
    rng = np.random.default_rng(3)
    wq = cases.random_weights(rng)
    params, lut = _off(1)
    params[0, 0], params[0, lo:lo + 25] = bit, wq
    img = np.zeros((1, 3, 11, 12), np.uint8)
    img[0, :, 5, 6] = 255
    out = oracle.augment(img, params, lut)[0][0, 0].astype(np.int64)
    want = ((wq.reshape(5, 5)[::-1, ::-1] * 255 + 32768) >> 16)
    assert np.array_equal(out[3:8, 4:9], want) and out.sum() == want.sum()
    # at the corner the reflection folds the weights: out(y, x) sums w[dy][dx] over every (dy, dx) with reflect(y + dy) = 0 = reflect(x + dx)
    img[:] = 0
    img[0, :, 0, 0] = 255
    out = oracle.augment(img, params, lut)[0][0, 0].astype(np.int64)
    W = wq.reshape(5, 5)
    assert out[0, 0] == (W[2, 2] * 255 + 32768) >> 16 and out[1, 1] == (W[1, 1] * 255 + 32768) >> 16
    assert out[2, 2] == (W[0, 0] * 255 + 32768) >> 16 and out[3:, :].sum() == 0
    img[:] = 0
    img[0, :, 1, 1] = 255  # (1,1) is reached from (0,0) by (1,1) and, reflected, by (-1,-1) -> (1,1), (-1,1), (1,-1)
    out = oracle.augment(img, params, lut)[0][0, 0].astype(np.int64)
    assert out[0, 0] == ((W[3, 3] + W[1, 1] + W[1, 3] + W[3, 1]) * 255 + 32768) >> 16


def test_invert_twice_is_the_identity_table():
    t = np.arange(256)
    once = oracle.table_step(t, lambda v: 255.0 - v)
    assert np.array_equal(oracle.table_step(once, lambda v: 255.0 - v), t) and once[0] == 255
    assert oracle.table_step(t, lambda v: v * 1.4)[-1] == 255 and oracle.table_step(t, lambda v: v - 25)[0] == 0
    assert oracle.table_step(np.array([2, 3]), lambda v: v * 0.5).tolist() == [1, 2]  # 1.0, 1.5 -> 2: half to even


def test_salt_and_dropout_rates_and_channels():
    crops = np.full((1, 3, 64, 64), 100, np.uint8)
    params, lut = _off(1)
    params[0, 0], params[0, 2] = cases.SALT, int(0.05 * 2 ** 32)
    out = oracle.augment(crops, params, lut, seed=9)[0][0]
    hit = out[0] != 100
    assert (out[0] == out[1]).all() and (out[0] == out[2]).all() and set(np.unique(out[0])) == {0, 100, 255}
    assert abs(hit.mean() - 0.05) < 4 * math.sqrt(0.05 * 0.95 / 4096)
    params[0, 0], params[0, 3], params[0, 4], params[0, 5] = cases.DROPOUT, int(0.45 * 2 ** 32), 3, 2
    out = oracle.augment(crops, params, lut, seed=9)[0][0]
    cells = {(y * 3 // 64, x * 2 // 64): int(out[0, y, x]) for y in range(64) for x in range(64)}
    assert all(out[0, y, x] == cells[(y * 3 // 64, x * 2 // 64)] for y in range(0, 64, 7) for x in range(0, 64, 5)) and set(cells.values()) <= {0, 100}


# ---- draw


CFG_ALL = dict(use_peper_salt=True, use_motion_blur=True, use_invert=True)


def test_draw_is_per_seed_and_sample():
    from lc_amd import augment

    cfg = augment.AugmentConfig(**CFG_ALL)
    ids = np.arange(40)
    P, L = augment.draw(cfg, 11, ids, 5, hw=(64, 96))
    perm = np.random.default_rng(0).permutation(40)[:17]
    P2, L2 = augment.draw(cfg, 11, ids[perm], 5, hw=(64, 96))
    assert np.array_equal(P2, P[perm]) and np.array_equal(L2, L[perm]) and P.dtype == np.int32 and L.dtype == np.uint8
    P3, _ = augment.draw(cfg, 12, ids, 5, hw=(64, 96))
    assert not np.array_equal(P3, P)
    assert (P[:, 56:] == 0).all() and (P[:, 0] & ~63 == 0).all()
    for row in P:
        augment.check_params(row[None], 64, 96, 5, True)
        for bit, lo in ((4, 6), (16, 31)):
            if row[0] & bit:
                assert row[lo:lo + 25].min() >= 0 and row[lo:lo + 25].sum() == 65536
        if row[0] & 8:
            assert (row[4], row[5]) == (3, 4) and row[3] == int(0.1 * 2 ** 32)
    # no backgrounds: never switched; the defaults of _gen_color_aug: no salt, no motion blur
    P4, _ = augment.draw(augment.AugmentConfig(), 11, ids, 0)
    assert not (P4[:, 0] & 7).any()
    assert np.array_equal(augment.key(11, ids, 7, 3), [oracle.key(11, i, 7, 3) for i in ids])


def test_draw_matches_the_restated_builders():
    from lc_amd import augment

    cfg = augment.AugmentConfig(pixel_aug_prob=1.0, **CFG_ALL)
    seed, ids = 77, np.arange(64)
    P, L = augment.draw(cfg, seed, ids, 3)
    seen = set()
    for i in ids:
        uu = lambda op, j: oracle.u(seed, i, oracle.OP_HOST + op, j)  # noqa: E731
        if P[i, 0] & 4:
            assert np.array_equal(P[i, 6:31], oracle.motion_weights(360.0 * uu(4, 1), 2.0 * uu(4, 2) - 1.0)), i
            seen.add("motion")
        if P[i, 0] & 16:
            assert np.array_equal(P[i, 31:56], oracle.gaussian_weights(1.2 * uu(6, 1))), i
            seen.add("gauss")
        if P[i, 0] & 1:
            assert P[i, 1] == min(int(uu(1, 1) * 3), 2)
        want = np.tile(np.arange(256), (3, 1))
        for c in range(3):
            t = want[c]
            pc = lambda op, prob: uu(op, 2 + c) if uu(op, 1) < prob else uu(op, 2)  # noqa: E731
            if uu(7, 0) < 0.5:
                t = oracle.table_step(t, lambda v: v + min(-25 + math.floor(pc(7, 0.3) * 51.0), 25))
            if uu(8, 0) < 0.4 and uu(8, 1 + c) < 0.2:
                t = oracle.table_step(t, lambda v: 255.0 - v)
            if uu(9, 0) < 0.5:
                t = oracle.table_step(t, lambda v: v * (0.6 + 0.8 * pc(9, 0.5)))
            if uu(10, 0) < 0.5:
                t = oracle.table_step(t, lambda v: v * (0.6 + 0.8 * uu(10, 1)))
            if uu(11, 0) < 0.5:
                t = oracle.table_step(t, lambda v: 128.0 + (0.5 + 1.7 * pc(11, 0.3)) * (v - 128.0))
            want[c] = t
        assert np.array_equal(L[i], want), i
    assert seen == {"motion", "gauss"}
    g = oracle.gaussian_weights(0.6).reshape(5, 5)
    assert np.array_equal(g, g.T) and np.array_equal(g, g[::-1]) and g[2, 2] == g.max() and g.sum() == 65536
    m = oracle.motion_weights(0.0, 0.0).reshape(5, 5)  # straight up and down, even weights: the centre column
    assert m[:, 2].sum() == 65536 and abs(int(m[0, 2]) - 13107) <= 1


def test_gate_frequencies_over_4096_samples():
    """Each gate within four binomial standard deviations of its probability at ONE fixed seed: deterministic, so it cannot flake."""
    from lc_amd import augment

    cfg = augment.AugmentConfig(**CFG_ALL)
    seed, ids = 2024, np.arange(4096)
    P, _ = augment.draw(cfg, seed, ids, 4)
    bits = P[:, 0]

    def within(hits, n, p):
        return abs(hits - n * p) <= 4 * math.sqrt(n * p * (1 - p))

    assert within(int((bits & 1 != 0).sum()), 4096, cfg.switch_bg_prob)
    chain = augment.u(seed, ids, augment.OP_CHAIN, 0) < cfg.pixel_aug_prob
    n = int(chain.sum())
    assert within(n, 4096, cfg.pixel_aug_prob) and not (bits[~chain] & 62).any()  # the chain's gate holds everything behind it
    for bit, p in ((2, 0.3), (4, 0.2), (8, 0.5), (16, 0.5 * (1 - 1e-3 / 1.2)), (32, 1 - 0.5 ** 4 * 0.6)):
        assert within(int((bits[chain] & bit != 0).sum()), n, p), (bit, p)
    g = P[bits & 1 != 0, 1]
    assert all(within(int((g == k).sum()), len(g), 0.25) for k in range(4))


# ---- the library


def test_build_group_header_exports_and_source_hash():
    from lc_amd import augment, build

    T = build.AUGMENT  # (its place among the libraries, its files and includes: tests/test_libraries_host.py)
    lib = augment.load()
    assert not build.is_stale(T)
    assert lib.lc_amd_augment_source_hash().decode() == build.source_hash(T) == build.embedded_hash(T.so_path, T.hash_marker)
    assert build.sources(T) == [os.path.join(build.CSRC, "augment", "lc_augment.hip")]

    header = open(os.path.join(ROOT, "include", "lc_amd_augment.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    declared = set(re.findall(r"\b(lc_[a-z0-9_]+)\s*\(", text))
    assert declared == set(augment._SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", T.so_path], capture_output=True, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert exported == declared, exported ^ declared
    assert lib.lc_amd_augment_version() == int(re.search(r"#define LC_AMD_AUGMENT_VERSION (\d+)", header).group(1)) == 1
    for name, have in (("MIN_SIZE", augment.MIN_SIZE), ("MAX_SIZE", augment.MAX_SIZE), ("WORDS", augment.WORDS), ("U8", augment.OUT_DTYPES[torch.uint8]),
                       ("F32", augment.OUT_DTYPES[torch.float32]), ("F16", augment.OUT_DTYPES[torch.float16]), ("BF16", augment.OUT_DTYPES[torch.bfloat16]),
                       ("FILTERED", augment.FORMS["filtered"]), ("POINTWISE", augment.FORMS["pointwise"]), ("OP_SNP", augment.OP_SNP),
                       ("OP_SNPV", augment.OP_SNPV), ("OP_DROP", augment.OP_DROP), ("OP_HOST", augment.OP_HOST)):
        assert have == int(re.search(rf"#define LC_AUGMENT_{name} (\d+)", header).group(1)), name
    assert (oracle.OP_SNP, oracle.OP_SNPV, oracle.OP_DROP, oracle.OP_HOST) == (augment.OP_SNP, augment.OP_SNPV, augment.OP_DROP, augment.OP_HOST)
    from lc_amd import maskcrop

    ops = {augment.OP_SNP, augment.OP_SNPV, augment.OP_DROP} | {v for k, v in vars(augment).items() if k.startswith("OP_") and k != "OP_HOST"}
    assert len(ops) == 16 and min(ops) > maskcrop.MAX_CHECK  # distinct, and above every round number of maskcrop's key
    kinds_of = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_uint64: "8", augment._FLOATS: "p"}
    m = re.search(r"int lc_augment_u8\((.*?)\);", text, flags=re.S)
    kinds = ["p" if "*" in a else {"int": "i", "uint64_t": "8"}[a.split()[0]] for a in m.group(1).split(",")]
    res, args = augment._SIGNATURES["lc_augment_u8"]
    assert res is ctypes.c_int and kinds == [kinds_of[a] for a in args], kinds


def test_eight_kernels_without_scratch_within_16_kb_of_lds(capsys):
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    from kernel_resources import kernel_resources

    from lc_amd import augment, build
    from tests.test_gpu_augment import KERNEL_FORMS

    augment.load()
    res = kernel_resources(build.AUGMENT.so_path)
    assert len(res) == 8 and all("lc_augment_" in n for n in res), sorted(res)
    for d in res.values():
        with capsys.disabled():
            print(f"\n{d['name']}: {d.get('group_segment_fixed_size', 0)} B of LDS, {d['vgpr_count']} VGPRs", end="")
        assert d.get("private_segment_fixed_size", 0) == 0 and d.get("vgpr_spill_count", 0) == 0 and d.get("sgpr_spill_count", 0) == 0, (d["name"], "scratch")
        assert d.get("group_segment_fixed_size", 0) <= 16 * 1024, d["name"]
    # the table of tests/test_gpu_augment.py: every form has exactly one entry, and the test it names exists there
    import ast

    tree = ast.parse(open(os.path.join(ROOT, "tests", "test_gpu_augment.py")).read())
    defined = {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}
    assert len(KERNEL_FORMS) == 8
    for name in res:
        assert sum(1 for rx in KERNEL_FORMS if re.search(rx, name)) == 1, name
    for rx, test in KERNEL_FORMS.items():
        assert any(re.search(rx, name) for name in res) and test in defined, (rx, test)


def test_entry_point_checks_its_arguments_before_launching():
    from lc_amd import augment

    lib = augment.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    three = (ctypes.c_float * 3)(1, 1, 1)

    def call(crops=p, bg=p, G=1, msk=p, params=p, lut=p, B=2, h=8, w=8, sid=None, dt=1, form=0, mean=None, std=None, out=p, info=p):
        return lib.lc_augment_u8(crops, bg, G, msk, params, lut, B, h, w, 0, sid, dt, form, mean, std, out, info, None)

    msg = lib.lc_amd_augment_last_error
    assert call(B=-1) != 0 and b"lc_augment_u8: B < 0" in msg()
    assert call(B=0) == 0 and call(B=0, crops=None, params=None, lut=None, out=None) == 0  # an empty batch is a no-op
    assert call(G=-1) != 0 and b"G < 0" in msg()
    assert call(h=7) != 0 and b"[8, 16384]" in msg() and call(w=16385) != 0 and b"16384" in msg()
    assert call(dt=4) != 0 and b"out_dtype" in msg() and call(dt=-1) != 0
    assert call(form=2) != 0 and b"form" in msg()
    assert call(mean=three) != 0 and b"come together" in msg()
    assert call(dt=0, mean=three, std=three) != 0 and b"float output" in msg()
    for name in ("crops", "params", "lut", "out"):
        assert call(**{name: None}) != 0 and b"NULL" in msg(), name
    assert call(bg=None) != 0 and b"backgrounds" in msg() and call(G=0) != 0 and b"backgrounds" in msg()
    assert call(params=p + 2) != 0 and b"aligned" in msg()
    assert call(lut=p + 1) != 0 and call(msk=p + 2) != 0 and call(sid=p + 1) != 0 and call(info=p + 2) != 0 and call(out=p + 2) != 0
    assert call(dt=2, out=p + 1) != 0 and b"aligned" in msg()
    assert call(B=2 ** 31 - 1, h=16384, w=16384) != 0 and b"too many" in msg()


def _good(B=2, h=8, w=9):
    params, lut = _off(B)
    return dict(crops=torch.zeros(B, 3, h, w, dtype=torch.uint8), params=params, lut=lut)


def test_wrapper_refusals():
    from lc_amd import augment

    f = augment.augment
    with pytest.raises(TypeError, match="crops must be a torch.Tensor"):
        f(**dict(_good(), crops=np.zeros((2, 3, 8, 9), np.uint8)))
    with pytest.raises(TypeError, match="crops must be uint8"):
        f(**dict(_good(), crops=torch.zeros(2, 3, 8, 9)))
    with pytest.raises(ValueError, match=r"crops has shape \(2, 1, 8, 9\)"):
        f(**dict(_good(), crops=torch.zeros(2, 1, 8, 9, dtype=torch.uint8)))
    with pytest.raises(ValueError, match="crop sizes of 8 to 16384, got 7 x 9"):
        f(**_good(h=7))
    with pytest.raises(TypeError, match="params must be int32"):
        f(**dict(_good(), params=np.zeros((2, 64), np.int64)))
    with pytest.raises(ValueError, match=r"params has shape \(2, 63\)"):
        f(**dict(_good(), params=np.zeros((2, 63), np.int32)))
    with pytest.raises(TypeError, match="lut must be uint8"):
        f(**dict(_good(), lut=np.zeros((2, 3, 256), np.int32)))
    with pytest.raises(ValueError, match=r"lut has shape \(1, 3, 256\)"):
        f(**dict(_good(), lut=np.zeros((1, 3, 256), np.uint8)))
    with pytest.raises(TypeError, match="msk_in must be float32"):
        f(**_good(), msk_in=torch.zeros(2, 8, 9, dtype=torch.float64))
    with pytest.raises(ValueError, match=r"msk_in has shape \(2, 9, 8\)"):
        f(**_good(), msk_in=torch.zeros(2, 9, 8))
    with pytest.raises(ValueError, match=r"backgrounds has shape \(4, 3, 8, 8\)"):
        f(**_good(), backgrounds=torch.zeros(4, 3, 8, 8, dtype=torch.uint8))
    with pytest.raises(TypeError, match="sample_id must be int32"):
        f(**_good(), sample_id=torch.zeros(2, dtype=torch.int64))
    with pytest.raises(ValueError, match="seed of 0 to"):
        f(**_good(), seed=2 ** 64)
    with pytest.raises(TypeError, match="seed must be a whole number"):
        f(**_good(), seed=1.0)
    with pytest.raises(TypeError, match="dtype must be one of"):
        f(**_good(), dtype=torch.float64)
    with pytest.raises(TypeError, match="normalize needs a float dtype"):
        f(**_good(), dtype=torch.uint8, normalize=(cases.MEAN, cases.STD))
    with pytest.raises(ValueError, match="one value per channel"):
        f(**_good(), normalize=((0.5,), cases.STD))
    with pytest.raises(TypeError, match="pointwise must be"):
        f(**_good(), pointwise=1)

    # the row rules, on host params, before anything is uploaded
    def bad(**words):
        g = _good()
        for j, v in words.items():
            g["params"][1, int(j[1:])] = v
        return g

    bgs, msk = torch.zeros(2, 3, 8, 9, dtype=torch.uint8), torch.zeros(2, 8, 9)
    with pytest.raises(ValueError, match="row 1 sets bits above bit 5"):
        f(**bad(w0=64))
    with pytest.raises(ValueError, match="row 1 has a non-zero reserved word"):
        f(**bad(w60=1))
    with pytest.raises(ValueError, match="filter A must be non-negative and sum to 65536, got a sum of 65535"):
        f(**bad(w0=4, w18=65535))
    with pytest.raises(ValueError, match="filter B must be non-negative and sum to 65536, got a sum of 65536 and a minimum of -1"):
        f(**bad(w0=16, w31=-1, w43=65537))
    with pytest.raises(ValueError, match="dropout grid of 1 x 1 to 8 x 9, got 0 x 3"):
        f(**bad(w0=8, w5=3))
    with pytest.raises(ValueError, match="got 2 x 10"):
        f(**bad(w0=8, w4=2, w5=10))
    with pytest.raises(ValueError, match="needs msk_in and backgrounds"):
        f(**bad(w0=1))
    with pytest.raises(ValueError, match="needs msk_in and backgrounds"):
        f(**bad(w0=1), backgrounds=bgs)
    with pytest.raises(ValueError, match="names background 2 of 2"):
        f(**bad(w0=1, w1=2), backgrounds=bgs, msk_in=msk)
    with pytest.raises(ValueError, match="pointwise=True, but a row"):
        f(**bad(w0=16, w43=65536), pointwise=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # everything in order: the crops are not on the HIP device
        f(**bad(w0=1 | 16, w1=1, w43=65536), backgrounds=bgs, msk_in=msk, sample_id=torch.zeros(2, dtype=torch.int32), normalize=(cases.MEAN, cases.STD))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(**_good())
    assert augment.check_params(bad(w0=16, w43=65536)["params"], 8, 9, 0, False) is True and augment.check_params(_off(2)[0], 8, 9, 0, False) is False


# ---- the two helpers against the reference's formulas, written out with the same u


def test_background_matrices_follow_switch_bg():
    from lc_amd import augment

    seed, ids, (H, W) = 31, [4, 9, 200, 7, 1], (64, 48)
    for hb, wb in ((480, 640), (50, 700), (64, 48), (300, 40)):
        M = augment.background_matrices(seed, ids, (hb, wb), (H, W))
        assert M.shape == (5, 2, 3) and M.dtype == np.float32
        for row, i in zip(M, ids):
            r = [oracle.u(seed, i, oracle.OP_HOST + 12, j) for j in range(4)]
            bg_roi_w = max(int(r[0] * wb), W)               # dataset.py:142-146
            bg_roi_h = max(int(r[1] * hb), H)
            bg_roi_l = max(int(r[2] * (wb - bg_roi_w)), 0)
            bg_roi_t = max(int(r[3] * (hb - bg_roi_h)), 0)
            rows = range(hb)[bg_roi_t:bg_roi_t + bg_roi_h]
            cols = range(wb)[bg_roi_l:bg_roi_l + bg_roi_l + bg_roi_w]
            fx, fy = W / len(cols), H / len(rows)
            want = np.array([[fx, 0, (0.5 - cols[0]) * fx - 0.5], [0, fy, (0.5 - rows[0]) * fy - 0.5]], dtype=np.float32)
            assert np.array_equal(row, want), (hb, wb, i)
            # cv2.resize's convention: the centre of the first crop pixel comes from region_w / W / 2 - 1/2 pixels into the region
            x_src = (0 - row[0, 2]) / row[0, 0]
            assert abs(x_src - (cols[0] + 0.5 * len(cols) / W - 0.5)) < 1e-3


def test_draw_zoom_follows_aug_bbox():
    from lc_amd import augment

    cfg = augment.AugmentConfig(rotate_prob=0.5)
    seed, ids = 5, np.arange(32)
    boxes = np.stack([np.array([10.0 + i, 20.0, 110.0 + 3 * i, 90.0 + i]) for i in ids])
    boxes[3] = [0, 0, 640, 100]  # the scale is capped by the frame
    centre, scale, rot = augment.draw_zoom(cfg, seed, ids, boxes, (480, 640))
    for i in ids:
        r = [oracle.u(seed, i, oracle.OP_HOST + 13, j) for j in range(5)]
        x1, y1, x2, y2 = boxes[i]
        cx, cy, bh, bw = 0.5 * (x1 + x2), 0.5 * (y1 + y2), y2 - y1, x2 - x1
        scale_ratio = 1 + cfg.dzi_scale_ratio * (2 * r[0] - 1)              # dataset.py:321-326
        shift_ratio = cfg.dzi_shift_ratio * (2 * np.array(r[1:3]) - 1)
        want_c = np.array([cx + bw * shift_ratio[0], cy + bh * shift_ratio[1]])
        want_s = min(max(y2 - y1, x2 - x1) * scale_ratio * cfg.dzi_pad_scale, max(480, 640)) * 1.0
        want_r = r[4] * 4 * math.pi if r[3] < cfg.rotate_prob else 0         # dataset.py:402
        assert np.array_equal(centre[i], want_c) and scale[i] == want_s and rot[i] == want_r, i
    assert scale[3] == 640 and 0 < (rot == 0).sum() < 32
    from lc_amd import crops

    M, Mi = crops.affine_from_box(centre[0], scale[0], rot[0], (64, 64))
    assert M.shape == (2, 3) and np.isfinite(M).all()
