"""Label preparation without a GPU: the argument checks of lc_sym_select_f32 / lc_label_targets_f32, the host-side chunk table of a
ragged candidate list, and the drop-in's opt-in rebinding of the reference's label-preparation names."""
import ctypes
import os
import sys

import pytest
import torch


def _ints(v):
    return (ctypes.c_int * len(v))(*v)


def test_sym_select_checks_its_arguments_before_launching():
    from lc_amd import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)

    def call(rows, ks, mode=1, a=p, b=p, B=None, N=64, H=8, W=8, ck=p, xyz_map=None, noc_scale=None, homo_z=None, dtype=0, bs=0, out=p):
        B = rows[-1] if B is None else B
        return lib.lc_sym_select_f32(p, _ints(rows), _ints(ks), len(ks), mode, p, a, b, xyz_map, dtype, bs, noc_scale, homo_z, ck, B, N, H, W, out,
                                     None, None)

    def err():
        return lib.lc_amd_last_error()

    assert call([0, 2, 5], [1, 4], B=5, N=1025) != 0 and b"1024" in err()
    assert call([0, 5], [4], mode=2) != 0 and b"mode" in err()
    assert call([0, 2, 5], [1, 4], B=6) != 0 and b"end at B" in err()
    assert call([0, 3, 2, 5], [1, 2, 4]) != 0 and b"decrease" in err()
    assert call([0, 2, 5], [1, 0]) != 0 and b"at least one candidate" in err()
    assert lib.lc_sym_select_f32(p, _ints([0] * 34), _ints([1] * 33), 33, 1, p, p, p, None, 0, 0, None, None, p, 0, 4, 8, 8, p, None, None) != 0
    assert b"32" in err()
    assert call([0, 5], [4], mode=0, b=None) != 0 and b"2D" in err()
    assert call([0, 5], [4], a=None) != 0 and b"noc_scale" in err()
    assert call([0, 5], [4], b=None) != 0 and b"homo_z" in err()
    assert call([0, 5], [4], b=None, homo_z=p, ck=None) != 0 and b"check pixels" in err()
    assert call([0, 5], [4], a=None, xyz_map=p, noc_scale=p, dtype=3) != 0 and b"map_dtype" in err()
    assert call([0, 5], [4], a=None, xyz_map=p, noc_scale=p, bs=10) != 0 and b"stride" in err()
    assert call([0, 5], [4], out=None) != 0 and b"null" in err()
    # an empty batch is a no-op (nothing is read or launched; the pointers are never touched)
    assert lib.lc_sym_select_f32(None, _ints([0, 0]), _ints([4]), 1, 1, None, None, None, None, 0, 0, None, None, None, 0, 64, 0, 0, None, None,
                                 None) == 0


def test_label_targets_checks_its_arguments_before_launching():
    from lc_amd import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)

    def call(B=2, H=4, W=4, bits=(7, 7, 6), m8=p, mf=None, sc=p, xyz=p, noc=None, tgt=p, raw=p, hz=p):
        return lib.lc_label_targets_f32(hz, m8, mf, p, p, sc, None, B, H, W, *bits, 1, xyz, noc, tgt, raw, None)

    def err():
        return lib.lc_amd_last_error()

    assert call(H=0) != 0 and b"size" in err()
    assert call(bits=(7, 0, 6)) != 0 and b"1..24" in err()
    assert call(bits=(7, 25, 6)) != 0 and b"1..24" in err()
    assert call(mf=p) != 0 and b"mask" in err()
    assert call(xyz=None, tgt=None, raw=None) != 0 and b"no output" in err()
    assert call(sc=None) != 0 and b"noc_scale" in err()
    assert call(hz=None) != 0 and b"null" in err()
    assert call(B=1 << 20, H=64, W=64) != 0 and b"2^31" in err()
    assert lib.lc_label_targets_f32(p + 2, None, None, p, p, None, None, 2, 4, 4, 0, 0, 0, 1, p, None, None, None, None) != 0
    assert b"aligned" in err()
    assert call(B=0, hz=None, sc=None) == 0  # empty batch: no-op


def test_chunk_table_of_ragged_candidate_lists():
    from lc_amd.labels import chunk_table

    c = [torch.zeros(2, 1, 3, 4), torch.zeros(0, 2, 3, 4), torch.zeros(3, 4, 3, 4), torch.zeros(1, 384, 3, 4)]
    rows, ks, offs, B, ktot = chunk_table(c)
    assert rows == [0, 2, 2, 5, 6] and ks == [1, 2, 4, 384] and offs == [0, 2, 2, 14] and B == 6 and ktot == 398
    assert ktot == sum(x.shape[0] * x.shape[1] for x in c)
    # the rows' candidates in the concatenated array, as the kernel finds them
    flat = torch.cat([x.reshape(-1, 3, 4) for x in c])
    assert flat.shape[0] == ktot
    with pytest.raises(ValueError):
        chunk_table([torch.zeros(2, 3, 4)])


_STAND_IN = {
    "losses.py": "def annots_on_the_fly(*a):\n    return 'ref'\n\ndef selete_best_pose(*a):\n    return 'ref'\n\n"
                 "def xyz_from_homo_z(*a):\n    return 'ref'\n",
    "symmetry.py": "def select_pose_2d(*a):\n    return 'ref'\n\ndef select_pose_3d(*a):\n    return 'ref'\n",
}
_NAMES = {"losses": ("annots_on_the_fly", "selete_best_pose", "xyz_from_homo_z"), "symmetry": ("select_pose_2d", "select_pose_3d")}


@pytest.fixture
def stand_in_reference(monkeypatch, tmp_path):
    for name, text in _STAND_IN.items():
        (tmp_path / name).write_text(text)
    monkeypatch.setattr(sys, "path", [str(tmp_path)] + list(sys.path))
    for name in ("losses", "symmetry"):
        monkeypatch.delitem(sys.modules, name, raising=False)
    before = dict(sys.modules)
    yield tmp_path
    for name in set(sys.modules) - set(before):  # install() registers modules under the reference's names: none of them outlive the test
        del sys.modules[name]
    sys.modules.update(before)


def test_install_native_labels_rebinds_the_reference_names(stand_in_reference):
    import importlib

    from lc_amd import dropin, labels

    done = dropin.install(patch_ptnet=False, gpu_initialiser=False, native_labels=True)
    assert done["labels"] is True
    for mod, attrs in _NAMES.items():
        m = importlib.import_module(mod)
        assert os.path.dirname(os.path.abspath(m.__file__)) == str(stand_in_reference)
        for a in attrs:
            assert getattr(m, a) is getattr(labels, a), (mod, a)


def test_install_without_the_flag_leaves_label_names_alone(stand_in_reference):
    import importlib

    from lc_amd import dropin

    done = dropin.install(patch_ptnet=False, gpu_initialiser=False)
    assert "labels" not in done
    for mod, attrs in _NAMES.items():
        m = importlib.import_module(mod)
        for a in attrs:
            assert getattr(m, a)() == "ref", (mod, a)


def test_dropin_command_line_flag(monkeypatch, tmp_path):
    from lc_amd import dropin

    seen = {}
    script = tmp_path / "train.py"
    script.write_text("import sys\nSEEN = list(sys.argv)\n")
    monkeypatch.setattr(dropin, "install", lambda **kw: seen.update(kw) or {})
    monkeypatch.setattr(sys, "argv", list(sys.argv))
    monkeypatch.setattr(sys, "path", list(sys.path))
    dropin.main(["--native-labels", str(script), "--cfg", "x.yaml"])
    assert seen == {"native_labels": True} and sys.argv == [str(script), "--cfg", "x.yaml"]
    seen.clear()
    dropin.main([str(script)])
    assert seen == {"native_labels": False}
