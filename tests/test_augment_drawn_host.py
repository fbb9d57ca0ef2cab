"""The drawn augmentation without a GPU: the header declares `lc_augment_drawn_u8`, its ctypes kinds and the draw-configuration struct
agree between the header and Python, the host op codes are the module's, and every argument rule of the entry point is refused before
anything is launched (host pointers that are never read)."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
C_TYPES = {"double": ctypes.c_double, "int": ctypes.c_int}


def _header():
    text = open(os.path.join(ROOT, "include", "lc_amd_augment.h")).read()
    return text, re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_declares_the_entry_point_and_ctypes_follows_the_prototype():
    from lc_amd import augment

    _, code = _header()
    m = re.search(r"int lc_augment_drawn_u8\((.*?)\);", code, flags=re.S)
    assert m, "include/lc_amd_augment.h does not declare lc_augment_drawn_u8"
    kinds = ["p" if "*" in a else {"int": "i", "uint64_t": "8", "lc_augment_draw_config": "cfg"}[a.split()[0]] for a in m.group(1).split(",")]
    kinds_of = {ctypes.c_void_p: "p", ctypes.c_int: "i", ctypes.c_uint64: "8", augment._FLOATS: "p", augment.DrawConfig: "cfg"}
    res, args = augment._SIGNATURES["lc_augment_drawn_u8"]
    assert res is ctypes.c_int and kinds == [kinds_of[a] for a in args], kinds
    assert kinds.count("cfg") == 1 and len(kinds) == 18
    # the existing entry point and the version are as they were
    assert re.search(r"#define LC_AMD_AUGMENT_VERSION 1\b", code)
    assert re.search(r"int lc_augment_u8\(const unsigned char \*crops, const unsigned char \*backgrounds, int G, const float \*msk_in, const int \*params,", code)
    lib = augment.load()
    assert lib.lc_amd_augment_version() == 1 and hasattr(lib, "lc_augment_drawn_u8")


def test_draw_config_struct_agrees_between_header_and_python():
    from lc_amd import augment

    _, code = _header()
    m = re.search(r"typedef struct lc_augment_draw_config \{(.*?)\} lc_augment_draw_config;", code, flags=re.S)
    assert m
    fields = [(name, C_TYPES[ctype]) for ctype, name in re.findall(r"(\w+) (\w+);", m.group(1))]
    assert fields == list(augment.DrawConfig._fields_)
    # the size a C compiler gives it: two doubles, four ints, no padding (every member lies on its own alignment)
    assert ctypes.sizeof(augment.DrawConfig) == 2 * 8 + 4 * 4 == 32 and ctypes.alignment(augment.DrawConfig) == 8
    offsets = [getattr(augment.DrawConfig, n).offset for n, _ in fields]
    assert offsets == [0, 8, 16, 20, 24, 28]
    # every field of AugmentConfig that `draw` reads is there, under its own name, and n_backgrounds besides
    names = [n for n, _ in fields]
    assert names[:-1] == [f for f in augment.AugmentConfig.__dataclass_fields__ if f in names] and names[-1] == "n_backgrounds"
    assert set(names[:-1]) == {"pixel_aug_prob", "switch_bg_prob", "use_peper_salt", "use_motion_blur", "use_invert"}


def test_header_op_codes_are_the_modules():
    from lc_amd import augment

    text, _ = _header()
    ops = {k[3:]: v for k, v in vars(augment).items() if k.startswith("OP_")}
    assert len(ops) == 17  # the sixteen distinct codes and OP_HOST, their base
    for name, have in ops.items():
        m = re.search(rf"#define LC_AUGMENT_OP_{name} (\d+)\n", text)
        assert m and int(m.group(1)) == have, name
    assert len(re.findall(r"#define LC_AUGMENT_OP_\w+ ", text)) == 17


def test_entry_point_refuses_every_argument_rule_before_launching():
    from lc_amd import augment

    lib = augment.load()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) + 15) & ~15
    three = (ctypes.c_float * 3)(1, 1, 1)

    def call(crops=p, bg=p, G=2, msk=p, cfg=(0.8, 0.5, 1, 1, 1, 2), seed=p, sid=p, B=2, h=8, w=8, dt=1, mean=None, std=None, out=p, info=p, params_out=p,
             lut_out=p):
        return lib.lc_augment_drawn_u8(crops, bg, G, msk, augment.DrawConfig(*cfg), seed, sid, B, h, w, dt, mean, std, out, info, params_out, lut_out, None)

    msg = lib.lc_amd_augment_last_error
    # the rules of this entry point
    assert call(seed=None) != 0 and b"lc_augment_drawn_u8: seed must not be NULL" in msg()
    assert call(sid=None) != 0 and b"lc_augment_drawn_u8: sample_id must not be NULL" in msg()
    for bad in (-0.01, 1.01, float("nan"), float("inf")):
        assert call(cfg=(bad, 0.5, 0, 0, 0, 2)) != 0 and b"pixel_aug_prob must lie in [0, 1]" in msg(), bad
        assert call(cfg=(0.8, bad, 0, 0, 0, 2)) != 0 and b"switch_bg_prob must lie in [0, 1]" in msg(), bad
    assert call(cfg=(0.8, 0.5, 0, 0, 0, 1), bg=None, G=0) != 0 and b"n_backgrounds = 1 without as many backgrounds (G = 0)" in msg()
    assert call(cfg=(0.8, 0.5, 0, 0, 0, 3)) != 0 and b"n_backgrounds = 3 without as many backgrounds (G = 2)" in msg()
    assert call(cfg=(0.8, 0.5, 0, 0, 0, -1)) != 0 and b"n_backgrounds = -1" in msg()
    assert call(seed=p + 4) != 0 and b"seed must be aligned to 8 bytes" in msg()
    assert call(params_out=p + 2) != 0 and b"aligned" in msg() and call(lut_out=p + 1) != 0 and b"aligned" in msg()
    # the rules it shares with lc_augment_u8, under its own name
    assert call(B=-1) != 0 and b"lc_augment_drawn_u8: B < 0" in msg()
    assert call(B=0) == 0 and call(B=0, crops=None, seed=None, sid=None, out=None) == 0  # an empty batch is a no-op
    assert call(G=-1) != 0 and b"G < 0" in msg()
    assert call(h=7) != 0 and b"[8, 16384]" in msg() and call(w=16385) != 0 and b"16384" in msg()
    assert call(dt=4) != 0 and b"out_dtype" in msg() and call(dt=-1) != 0
    assert call(mean=three) != 0 and b"come together" in msg()
    assert call(dt=0, mean=three, std=three) != 0 and b"float output" in msg()
    for name in ("crops", "out"):
        assert call(**{name: None}) != 0 and b"NULL" in msg(), name
    assert call(bg=None) != 0 and b"backgrounds" in msg() and call(G=0) != 0 and b"backgrounds" in msg()
    assert call(msk=p + 2) != 0 and b"aligned" in msg() and call(sid=p + 1) != 0 and call(info=p + 2) != 0 and call(out=p + 2) != 0
    assert call(dt=2, out=p + 1) != 0 and b"aligned" in msg()
    assert call(B=2 ** 31 - 1, h=16384, w=16384) != 0 and b"too many" in msg()
    # the probabilities' ends are allowed: nothing but the launch is left, which host pointers must not reach -- so only the rule is read here
    for ends in ((0.0, 0.0), (1.0, 1.0)):
        assert call(cfg=(*ends, 0, 0, 0, 2), B=0) == 0


def test_the_gpu_tests_seeds_open_and_shut_every_gate():
    """tests/test_gpu_augment_drawn.py compares 67 drawn rows with `draw`: under the default probabilities each of the eleven gates is
    open in some of those rows and shut in others, for both of its seeds, and the five rows of its pixel test run every stage."""
    import numpy as np

    from lc_amd import augment
    from tests import test_gpu_augment_drawn as T

    cfg = augment.AugmentConfig(**T.CONFIGS["defaults_with_switches"])
    assert (cfg.pixel_aug_prob, cfg.switch_bg_prob) == (augment.AugmentConfig().pixel_aug_prob, augment.AugmentConfig().switch_bg_prob)
    assert len(T.IDS) == 67 and T.SEED >= 2 ** 32 and T.SEED2 >= 2 ** 32 and (T.IDS < 0).any() and len(set(T.IDS.tolist())) < 67
    for seed in (T.SEED, T.SEED2):
        chain = augment.u(seed, T.IDS, augment.OP_CHAIN, 0) < cfg.pixel_aug_prob
        gates = {"switch": augment.u(seed, T.IDS, augment.OP_SWITCH, 0) < cfg.switch_bg_prob, "chain": chain}
        for name, p in (("SALT", 0.3), ("MOTION", 0.2), ("DROPOUT", 0.5), ("GAUSS", 0.5), ("ADD", 0.5), ("INVERT", 0.4), ("MUL_PC", 0.5), ("MUL", 0.5),
                        ("CONTRAST", 0.5)):
            gates[name] = chain & (augment.u(seed, T.IDS, getattr(augment, "OP_" + name), 0) < p)
        assert len(gates) == 11
        for name, open_ in gates.items():
            assert 0 < int(open_.sum()) < 67, (seed, name)
        bits = augment.draw(cfg, seed, T.IDS, T.G, hw=(24, 40))[0][:, 0]  # the five stage bits follow their gates (sigma >= 1e-3 in every row)
        assert all(np.array_equal((bits & b) != 0, gates[n]) for b, n in ((1, "switch"), (2, "SALT"), (4, "MOTION"), (8, "DROPOUT"), (16, "GAUSS")))
    P, _ = augment.draw(augment.AugmentConfig(**T.ALL_ON), T.SEED, T.IDS[[0, 1, 2, 3, 5]], T.G, hw=(8, 8))
    assert int(np.bitwise_or.reduce(P[:, 0])) == 63


def _good(B=2, h=8, w=9):
    from lc_amd import augment

    return dict(crops=torch.zeros(B, 3, h, w, dtype=torch.uint8), cfg=augment.AugmentConfig(), seed=3, sample_id=torch.zeros(B, dtype=torch.int32))


def test_wrapper_refusals():
    from lc_amd import augment

    f = augment.augment_drawn
    with pytest.raises(TypeError, match="crops must be uint8"):
        f(**dict(_good(), crops=torch.zeros(2, 3, 8, 9)))
    with pytest.raises(ValueError, match="crop sizes of 8 to 16384, got 7 x 9"):
        f(**_good(h=7))
    with pytest.raises(TypeError, match="cfg must be an AugmentConfig"):
        f(**dict(_good(), cfg=dict(pixel_aug_prob=0.5)))
    with pytest.raises(ValueError, match=r"pixel_aug_prob must lie in \[0, 1\], got 1.5"):
        f(**dict(_good(), cfg=augment.AugmentConfig(pixel_aug_prob=1.5)))
    with pytest.raises(ValueError, match=r"switch_bg_prob must lie in \[0, 1\], got -0.1"):
        f(**dict(_good(), cfg=augment.AugmentConfig(switch_bg_prob=-0.1)))
    with pytest.raises(TypeError, match="needs sample_id"):
        f(**dict(_good(), sample_id=None))
    with pytest.raises(TypeError, match="sample_id must be int32"):
        f(**dict(_good(), sample_id=torch.zeros(2, dtype=torch.int64)))
    with pytest.raises(ValueError, match=r"sample_id has shape \(3,\)"):
        f(**dict(_good(), sample_id=torch.zeros(3, dtype=torch.int32)))
    with pytest.raises(ValueError, match="seed of 0 to"):
        f(**dict(_good(), seed=2 ** 64))
    with pytest.raises(TypeError, match="seed must be a whole number"):
        f(**dict(_good(), seed=1.0))
    with pytest.raises(TypeError, match="normalize needs a float dtype"):
        f(**_good(), dtype=torch.uint8, normalize=((0.5,) * 3, (0.2,) * 3))
    with pytest.raises(TypeError, match="dtype must be one of"):
        f(**_good(), dtype=torch.float64)
    with pytest.raises(ValueError, match=r"msk_in has shape \(2, 9, 8\)"):
        f(**_good(), msk_in=torch.zeros(2, 9, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):  # everything in order: the crops are not on the HIP device
        f(**_good())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        f(**dict(_good(), seed=torch.zeros(1, dtype=torch.int64)), return_rows=True)
