"""The shared binding layer without a GPU: every helper of `lc_amd._args.Args` (one accepting case, every refusing branch with its
exception type and whole message), the two settings of `whole` as the three modules use them, and `lc_amd._lib.SideLibrary`."""
import ctypes
import re

import numpy as np
import pytest
import torch

from lc_amd import _args, _lib

A = _args.Args("vsd")
G = _args.Args("gtinfo")


def refuses(exc, text):
    return pytest.raises(exc, match="^" + re.escape(text) + "$")


def test_tensor_f32_i32_rows():
    t = torch.zeros(3, 4, 5)
    assert A.tensor("x", t, (torch.float32,), "float32", (3, None, 5)) is t and A.f32("x", t, (None, None, None)) is t
    with refuses(TypeError, "lc_amd.vsd: x must be a torch.Tensor, got <class 'numpy.ndarray'>"):
        A.f32("x", np.zeros(3), (3,))
    with refuses(TypeError, "lc_amd.vsd: x must be float32, got torch.float64"):
        A.f32("x", t.double(), (3, 4, 5))
    with refuses(TypeError, "lc_amd.rle: masks must be uint8 or bool, got torch.float32"):
        _args.Args("rle").tensor("masks", t, (torch.uint8, torch.bool), "uint8 or bool", (None, None, None))
    with refuses(ValueError, "lc_amd.vsd: x has shape (3, 4, 5), expected (3, *, 6)"):
        A.f32("x", t, (3, None, 6))
    with refuses(ValueError, "lc_amd.vsd: x has shape (3, 4, 5), expected (*, *)"):
        A.f32("x", t, (None, None))
    with refuses(ValueError, "lc_amd.vsd: x has shape (3, 4, 5), expected (3)"):  # the starred form writes a one-entry shape without a comma
        A.f32("x", t, (3,))
    i = torch.zeros(3, dtype=torch.int64)
    assert A.i32("i", i, (3,)) is i and A.i32("i", i.int(), (3,)).dtype == torch.int32
    with refuses(TypeError, "lc_amd.vsd: i must be a torch.Tensor, got <class 'list'>"):
        A.i32("i", [0, 1, 2], (3,))
    with refuses(TypeError, "lc_amd.vsd: i must be int32 or int64, got torch.int16"):
        A.i32("i", i.short(), (3,))
    with refuses(ValueError, "lc_amd.vsd: i has shape (3,), expected (4,)"):  # the index form writes the tuple
        A.i32("i", i, (4,))
    with refuses(ValueError, "lc_amd.vsd: i has shape (3,), expected (3, 2)"):
        A.i32("i", i, (3, 2))
    P = _args.Args("posecov")
    assert P.rows("K", torch.zeros(2, 3, 3), (2, 3, 3)) is None
    with refuses(ValueError, "lc_amd.posecov: K has shape (2, 3, 3), expected (1, 3, 3)"):
        P.rows("K", torch.zeros(2, 3, 3), (1, 3, 3))


@pytest.mark.parametrize("numpy", [False, True])
def test_whole(numpy):
    M = _args.Args("maskcrop")
    assert M.whole("n", 3, 0, 5, numpy=numpy) == 3 and type(M.whole("n", 3, 0, 5, numpy=numpy)) is int
    assert M.whole("n", 0, 0, 5, numpy=numpy) == 0 and M.whole("n", 5, 0, 5, numpy=numpy) == 5
    with refuses(TypeError, "lc_amd.maskcrop: n must be a whole number, got <class 'bool'>"):
        M.whole("n", True, 0, 5, numpy=numpy)
    with refuses(TypeError, f"lc_amd.maskcrop: n must be a whole number, got {type(np.bool_(1))}"):
        M.whole("n", np.bool_(1), 0, 5, numpy=numpy)
    with refuses(TypeError, "lc_amd.maskcrop: n must be a whole number, got <class 'float'>"):
        M.whole("n", 3.0, 0, 5, numpy=numpy)
    if numpy:
        got = M.whole("n", np.int64(3), 0, 5, numpy=True)
        assert got == 3 and type(got) is int
        with refuses(ValueError, "lc_amd.maskcrop: n of 0 to 5, got 6"):
            M.whole("n", np.int64(6), 0, 5, numpy=True)
    else:
        with refuses(TypeError, "lc_amd.maskcrop: n must be a whole number, got <class 'numpy.int64'>"):
            M.whole("n", np.int64(3), 0, 5)
    with refuses(ValueError, "lc_amd.maskcrop: n of 0 to 5, got 6"):
        M.whole("n", 6, 0, 5, numpy=numpy)
    with refuses(ValueError, "lc_amd.maskcrop: n of 0 to 5, got -1"):
        M.whole("n", -1, 0, 5, numpy=numpy)


def test_each_module_keeps_its_whole_numbers():
    """maskcrop takes Python's whole numbers only; rle and augment take numpy's as well; none takes a bool.  Through the modules' own
    functions, which get this far (or past it, to the first rule that needs the device) on CPU tensors."""
    from lc_amd import augment, maskcrop, rle

    masks, M = torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(1, 2, 3)
    with refuses(TypeError, "lc_amd.maskcrop: n_check must be a whole number, got <class 'numpy.int64'>"):
        maskcrop.mask_crops(masks, M, (8, 8), n_check=np.int64(4))
    with refuses(TypeError, "lc_amd.maskcrop: out_hw must be a whole number, got <class 'numpy.int64'>"):
        maskcrop.mask_crops(masks, M, (np.int64(8), 8))
    with refuses(TypeError, "lc_amd.maskcrop: n_check must be a whole number, got <class 'bool'>"):
        maskcrop.mask_crops(masks, M, (8, 8), n_check=True)
    with pytest.raises(RuntimeError, match="lc_amd.maskcrop: masks is on cpu; the HIP path needs tensors on the MI355X"):
        maskcrop.mask_crops(masks, M, (8, 8), n_check=4)  # every host rule passed

    with pytest.raises(RuntimeError, match="lc_amd.rle: masks is on cpu; the HIP path needs tensors on the MI355X"):
        rle.encode(masks, cap=np.int64(4))  # accepted: the next refusal is the device's
    with refuses(TypeError, "lc_amd.rle: cap must be a whole number, got <class 'bool'>"):
        rle.encode(masks, cap=True)
    with refuses(TypeError, f"lc_amd.rle: cap must be a whole number, got {type(np.bool_(1))}"):
        rle.encode(masks, cap=np.bool_(1))
    with refuses(TypeError, "lc_amd.rle: cap must be a whole number, got <class 'float'>"):
        rle.encode(masks, cap=3.0)
    with refuses(ValueError, "lc_amd.rle: sizes of 1 to 16384, got 0"):
        rle.encode(masks, sizes=(np.int32(0), 8))

    cfg = augment.AugmentConfig()
    params, lut = augment.draw(cfg, np.int64(4), [0, 1], np.int64(0), hw=(np.int64(8), 8))  # accepted
    assert params.shape == (2, 64) and lut.shape == (2, 3, 256)
    assert np.array_equal(params, augment.draw(cfg, 4, [0, 1], 0, hw=(8, 8))[0])
    with refuses(TypeError, "lc_amd.augment: seed must be a whole number, got <class 'bool'>"):
        augment.draw(cfg, True, [0], 0)
    with refuses(TypeError, f"lc_amd.augment: seed must be a whole number, got {type(np.bool_(1))}"):
        augment.draw(cfg, np.bool_(1), [0], 0)
    with refuses(TypeError, "lc_amd.augment: n_backgrounds must be a whole number, got <class 'float'>"):
        augment.draw(cfg, 4, [0], 3.0)
    with refuses(ValueError, "lc_amd.augment: hw of 8 to 16384, got 7"):
        augment.draw(cfg, 4, [0], 0, hw=(np.int64(7), 8))


def test_pair_size_pair_center_delta_host_floats():
    assert G.pair("margin", (1, 2)) == (1, 2) and G.pair("margin", [3, 4]) == (3, 4)
    for bad in (torch.zeros(2), "ab", 7, (1, 2, 3)):
        with refuses(ValueError, f"lc_amd.gtinfo: margin is a pair, got {bad!r}"):
            G.pair("margin", bad)
    R = _args.Args("rle")
    assert R.size_pair("hw", (np.int64(4), 5), 16, numpy=True) == (4, 5) and R.size_pair("hw", (1, 16), 16) == (1, 16)
    with refuses(ValueError, "lc_amd.rle: hw is a pair, got 5"):
        R.size_pair("hw", 5, 16)
    with refuses(TypeError, "lc_amd.rle: hw must be a whole number, got <class 'float'>"):
        R.size_pair("hw", (4, 5.0), 16, numpy=True)
    with refuses(TypeError, "lc_amd.rle: hw must be a whole number, got <class 'numpy.int64'>"):
        R.size_pair("hw", (np.int64(4), 5), 16)
    with refuses(ValueError, "lc_amd.rle: hw of 1 to 16, got 17"):
        R.size_pair("hw", (17, 5), 16)
    with refuses(ValueError, "lc_amd.rle: hw of 1 to 16, got 0"):
        R.size_pair("hw", (4, 0), 16)

    assert G.center((0, 0.5)) == (0.0, 0.5) and A.center([1, 2], cx_cy=True) == (1.0, 2.0)
    with refuses(ValueError, "lc_amd.gtinfo: pixel_center is a pair, got 0.5"):
        G.center(0.5)
    with refuses(ValueError, "lc_amd.gtinfo: pixel_center is a pair, got (1, 2, 3)"):
        G.center((1, 2, 3))
    with refuses(ValueError, "lc_amd.gtinfo: pixel_center is a pair, got 'ab'"):
        G.center("ab")
    with refuses(ValueError, "lc_amd.vsd: pixel_center is a pair (cx, cy), got 0.5"):
        A.center(0.5, cx_cy=True)
    with refuses(ValueError, "lc_amd.vsd: pixel_center is a pair (cx, cy), got (1, 2, 3)"):
        A.center((1, 2, 3), cx_cy=True)
    assert A.center(torch.tensor([1.0, 2.0]), cx_cy=True) == (1.0, 2.0)  # the older form lets a two-element tensor through

    assert A.delta(15) == 15.0 and type(A.delta(15)) is float and A.delta(0.0) == 0.0
    with refuses(TypeError, "lc_amd.vsd: delta must be a number, got <class 'bool'>"):
        A.delta(True)
    with refuses(TypeError, "lc_amd.vsd: delta must be a number, got <class 'str'>"):
        A.delta("15")
    with refuses(ValueError, "lc_amd.vsd: delta must be finite and not negative, got -1"):
        A.delta(-1)
    with refuses(ValueError, "lc_amd.vsd: delta must be finite and not negative, got inf"):
        A.delta(float("inf"))
    with refuses(ValueError, "lc_amd.vsd: delta must be finite and not negative, got nan"):
        A.delta(float("nan"))

    C = _args.Args("crops")
    for x in ((0.5, 0.25, 0.125), np.asarray([0.5, 0.25, 0.125]), torch.tensor([[0.5], [0.25], [0.125]])):
        got = C.host_floats("mean", x, 3)
        assert isinstance(got, ctypes.c_float * 3) and list(got) == [0.5, 0.25, 0.125]
    assert list(C.host_floats("std", 2.0, 1)) == [2.0]
    with refuses(ValueError, "lc_amd.crops: normalize std must hold one value per channel (3), got 2"):
        C.host_floats("std", (1.0, 2.0), 3)
    with refuses(ValueError, "lc_amd.augment: normalize mean must hold one value per channel (3), got 1"):
        _args.Args("augment").host_floats("mean", 0.5, 3)


def test_same_device():
    cpu, meta = torch.device("cpu"), torch.device("meta")
    a, m = torch.zeros(2), torch.zeros(2, device=meta)
    assert A.same_device(cpu, "depth_est is on {}", depth_gt=a, K=a, diameter=None) is None
    with refuses(RuntimeError, "lc_amd.vsd: K is on meta, depth_est is on cpu"):
        A.same_device(cpu, "depth_est is on {}", depth_gt=a, K=m, diameter=m)  # the first one off the device is named
    with refuses(RuntimeError, "lc_amd.gtinfo: origin_xy is on cpu, depth_inst is on meta"):
        G.same_device(meta, "depth_inst is on {}", scene_index=m, origin_xy=a)
    with refuses(RuntimeError, "lc_amd.maskcrop: out['msk_vis'] is on meta, the masks on cpu"):
        _args.Args("maskcrop").same_device(cpu, "the masks on {}", M=a, **{"out['msk_vis']": m})
    with refuses(RuntimeError, "lc_amd.rle: out[1] is on meta, the store on cpu"):
        _args.Args("rle").same_device(cpu, "the store on {}", index=None, **{"out[0]": a, "out[1]": m})
    with refuses(RuntimeError, "lc_amd.posecov: pose is on meta, pts3d on cpu"):
        _args.Args("posecov").same_device(cpu, "pts3d on {}", pose=m)
    with refuses(RuntimeError, "lc_amd.metrics: t_gt is on meta, the poses are on cpu"):
        _args.Args("metrics").same_device(cpu, "the poses are on {}", t_gt=m)
    with refuses(RuntimeError, "lc_amd.gtinfo: R is on meta, the meshes are on cpu (there is no CPU fallback in the product path)"):
        G.same_device(cpu, _args.MESHES_ON, mesh_index=a, R=m)


def test_scenes_and_scene_index():
    d2, d3 = torch.zeros(4, 5), torch.zeros(3, 4, 5)
    Dt, S = A.scenes(d2, None, 3, "poses")
    assert tuple(Dt.shape) == (1, 4, 5) and S == 1 and Dt.data_ptr() == d2.data_ptr()
    assert A.scenes(d3, None, 3, "poses")[1] == 3 and A.scenes(d3, torch.zeros(7, dtype=torch.int64), 7, "poses")[1] == 3
    with refuses(TypeError, "lc_amd.vsd: depth_test must be a torch.Tensor, got <class 'NoneType'>"):
        A.scenes(None, None, 3, "poses")
    with refuses(TypeError, "lc_amd.vsd: depth_test must be float32, got torch.float16"):
        A.scenes(d3.half(), None, 3, "poses")
    with refuses(ValueError, "lc_amd.vsd: depth_test has shape (1, 3, 4, 5), expected (*, *, *)"):
        A.scenes(d3[None], None, 3, "poses")
    with refuses(ValueError, "lc_amd.vsd: scene_index is needed to tell which of the 3 scenes each of the 7 poses belongs to"):
        A.scenes(d3, None, 7, "poses")
    with refuses(ValueError, "lc_amd.gtinfo: scene_index is needed to tell which of the 3 scenes each of the 7 instances belongs to"):
        G.scenes(d3, None, 7, "instances")
    with refuses(TypeError, "lc_amd.vsd: scene_index must be int32 or int64, got torch.float32"):
        A.scenes(d3, torch.zeros(7), 7, "poses")
    with refuses(ValueError, "lc_amd.vsd: scene_index has shape (6,), expected (7,)"):
        A.scenes(d3, torch.zeros(6, dtype=torch.int32), 7, "poses")
    cpu = torch.device("cpu")
    one, each = A.scene_index(None, 1, 4, cpu), A.scene_index(None, 4, 4, cpu)
    assert one.dtype == each.dtype == torch.int32 and one.tolist() == [0, 0, 0, 0] and each.tolist() == [0, 1, 2, 3]
    given = torch.tensor([2, 0, 1], dtype=torch.int64)[::1]
    got = A.scene_index(given, 3, 3, cpu)
    assert got.dtype == torch.int32 and got.is_contiguous() and got.tolist() == [2, 0, 1]
    same = torch.tensor([2, 0, 1], dtype=torch.int32)
    assert A.scene_index(same, 3, 3, cpu).data_ptr() == same.data_ptr()  # nothing made where nothing is needed


def test_cam_K_and_pose_batch():
    eye = torch.eye(3)
    K = A.cam_K("K", eye, 4)
    assert tuple(K.shape) == (4, 3, 3) and K.data_ptr() == eye.data_ptr() and K.stride(0) == 0  # a view
    assert A.cam_K("K", torch.zeros(4, 3, 3), 4).stride(0) == 9
    with refuses(ValueError, "lc_amd.vsd: K has shape (2, 3, 3), expected (4, 3, 3)"):
        A.cam_K("K", torch.zeros(2, 3, 3), 4)
    with refuses(TypeError, "lc_amd.vsd: K must be float32, got torch.float64"):
        A.cam_K("K", eye.double(), 4)
    with refuses(TypeError, "lc_amd.vsd: K must be a torch.Tensor, got <class 'numpy.ndarray'>"):
        A.cam_K("K", np.eye(3, dtype=np.float32), 4)

    mi, R, t31, t3 = torch.zeros(4, dtype=torch.int32), torch.zeros(4, 3, 3), torch.zeros(4, 3, 1), torch.zeros(4, 3)
    B, (Re, Rg), (te, tg), Kc = A.pose_batch(mi, dict(R_est=R, R_gt=R), dict(t_est=t31, t_gt=t3), eye)
    assert B == 4 and Re is R and Rg is R and tuple(te.shape) == (4, 3) and te.data_ptr() == t31.data_ptr() and tg.data_ptr() == t3.data_ptr() and tuple(Kc.shape) == (4, 3, 3)
    B, (Rc,), (tc,), Kc = G.pose_batch(mi, dict(R=R), dict(t=t3), torch.zeros(4, 3, 3))
    assert B == 4 and Rc is R and tc.data_ptr() == t3.data_ptr() and tuple(tc.shape) == (4, 3)
    B, Rs, ts, Kc = A.pose_batch(None, dict(R_est=R, R_gt=R), dict(t_est=t3), eye, "cam_K")  # no mesh_index: the first R sets B
    assert B == 4 and len(Rs) == 2 and len(ts) == 1
    for bad in (mi.long(), [0, 1, 2, 3]):
        with refuses(TypeError, "lc_amd.vsd: mesh_index must be an int32 tensor on the GPU (MeshSet.index_of)"):
            A.pose_batch(bad, dict(R=R), dict(t=t3), eye)
    with refuses(ValueError, "lc_amd.gtinfo: mesh_index has shape (4, 1), expected (B,)"):
        G.pose_batch(mi[:, None], dict(R=R), dict(t=t3), eye)
    with refuses(ValueError, "lc_amd.vsd: R_gt has shape (3, 3, 3), expected (4, 3, 3)"):
        A.pose_batch(mi, dict(R_est=R, R_gt=R[:3]), dict(t_est=t3, t_gt=t3), eye)
    with refuses(TypeError, "lc_amd.vsd: R_est must be float32, got torch.float64"):
        A.pose_batch(mi, dict(R_est=R.double(), R_gt=R[:3]), dict(t_est=t3, t_gt=t3), eye)  # doubly wrong: the first rule speaks
    with refuses(ValueError, "lc_amd.vsd: t_gt has shape (4, 1, 3), expected (4, 3) or (4, 3, 1)"):
        A.pose_batch(mi, dict(R_est=R, R_gt=R), dict(t_est=t3, t_gt=t3[:, None]), eye)
    with refuses(ValueError, "lc_amd.vsd: t_gt has shape (12,), expected (4, 3) or (4, 3, 1)"):  # both shapes are judged before either element type
        A.pose_batch(mi, dict(R_est=R, R_gt=R), dict(t_est=t3.double(), t_gt=t3.reshape(12)), eye)
    with refuses(TypeError, "lc_amd.vsd: t_est must be float32, got torch.float64"):
        A.pose_batch(mi, dict(R_est=R, R_gt=R), dict(t_est=t3.double(), t_gt=t3), eye)
    with refuses(TypeError, "lc_amd.vsd: t_est must be a torch.Tensor, got <class 'numpy.ndarray'>"):
        A.pose_batch(mi, dict(R_est=R, R_gt=R), dict(t_est=np.zeros((4, 3), np.float32), t_gt=t3), eye)
    with refuses(ValueError, "lc_amd.metrics: cam_K has shape (2, 3, 3), expected (4, 3, 3)"):
        _args.Args("metrics").pose_batch(None, dict(R_est=R), dict(t_est=t3), torch.zeros(2, 3, 3), "cam_K")
    with refuses(ValueError, "lc_amd.metrics: R_est has shape (4, 3), expected (*, 3, 3)"):
        _args.Args("metrics").pose_batch(None, dict(R_est=t3), dict(t_est=t3), eye, "cam_K")
    seen = []
    A.pose_batch(None, dict(R_est=R), dict(t_est=t3), eye, "cam_K", lambda name, x, shape: (seen.append((name, shape)), x)[1])
    assert seen == [("R_est", (None, 3, 3)), ("t_est", (4, 3)), ("cam_K", (4, 3, 3))]  # the caller's own float check, in rule order


def test_side_library():
    from lc_amd import build

    entry = {"lc_x_f32": (ctypes.c_int, [ctypes.c_void_p])}
    x = _lib.SideLibrary(build.VSD._replace(name="x"), entry)
    assert x.signatures == {"lc_amd_x_version": (ctypes.c_int, []), "lc_amd_x_last_error": (ctypes.c_char_p, []),
                            "lc_amd_x_source_hash": (ctypes.c_char_p, []), **entry}
    assert list(x.signatures) == ["lc_amd_x_version", "lc_amd_x_last_error", "lc_amd_x_source_hash", "lc_x_f32"]

    from lc_amd import vsd

    so = _lib.SideLibrary(build.VSD, {"lc_vsd_score_f32": vsd._SIGNATURES["lc_vsd_score_f32"]})
    assert so.signatures == vsd._SIGNATURES and so.target is build.VSD
    lib = so.load()
    assert so.load() is lib and so.load(build_if_missing=False) is lib and lib.lc_amd_vsd_version() == 1  # cached
    assert vsd.load() is vsd.load()
    # a call the library refuses before any launch: null pointers and B < 0
    taus = (ctypes.c_float * 1)(0.1)
    rc = lib.lc_vsd_score_f32(None, None, None, None, None, None, taus, 1, 15.0, None, -1, 4, 4, 1, 4, 4, 0.0, 0.0, None, None, None)
    said = lib.lc_amd_vsd_last_error().decode()
    assert rc != 0 and said
    with refuses(RuntimeError, f"lc_amd.lc_vsd_score_f32 failed (code {rc}): {said}"):
        so.fail("lc_vsd_score_f32", rc)
    with refuses(RuntimeError, f"lc_amd.vsd.anything failed (code 7): {said}"):  # `what` is the module's own text after `lc_amd.`
        so.fail("vsd.anything", 7)
