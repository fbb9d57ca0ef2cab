"""CPU tests of the host layer: the C-ABI library's exports, the reference-surface semantics of cer_solver / Loss_fn /
NormClipper (against golden trajectories from the reference), and the drop-in installer.  Compute runs on the oracle
through tests/cpu_backend.py -- no HIP kernel is launched here."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.cpu_backend import oracle_backend  # noqa: F401
from tests.util import GOLDEN, rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_loads_and_exports_every_declared_symbol():
    from lc_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "lc_amd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(lc_[a-z0-9_]+|pnp_ceres_f32_omp)\s*\(", hdr))
    assert {"pnp_ceres_f32_omp", "lc_pnp_lm3_f32", "lc_cov_loss3_fwd_bwd_f32", "lc_pose_unit2_f32", "lc_softargmax2d_fwd", "lc_xyz_bin_loss_counts"} <= declared
    # one entry point per operation (LC_AMD_VERSION 2): no superseded generation is declared or exported any more
    retired = {"lc_pnp_lm_f32", "lc_pnp_lm2_f32", "lc_pnp_lm_chain_f32", "lc_cov_loss_fwd_bwd_f32", "lc_cov_loss2_fwd_bwd_f32", "lc_pose_unit_f32",
               "lc_softargmax2d_fwd_f32", "lc_dense_frontend_fwd_f32", "lc_dense_frontend_fwd2_f32", "lc_dense_frontend_select_f32",
               "lc_dense_frontend_select2", "lc_pnp_ransac_init_f32", "lc_pnp_ransac_init2_f32", "lc_pnp_ransac_init3_f32", "lc_pnp_ransac_init4_f32",
               "lc_bits_decode_f32", "lc_bits_decode2_f32", "lc_bits_decode_gt_fwd_f32", "lc_bits_decode_gt_fwd2_f32", "lc_sqnorm_f32",
               "lc_norm_clip_apply_f32", "lc_xyz_bin_loss_fwd_f32", "lc_dense_aux_fwd_f32"}
    assert not (retired & declared)
    lib = ctypes.CDLL(_lib.lib_path())
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/lc_amd.h but not exported"
    for name in retired:
        assert not hasattr(lib, name), f"{name} was retired but is still exported"
    assert set(_lib.EXPORTED_SYMBOLS) == declared
    assert _lib.load().lc_amd_version() == 2


def test_ransac_workspace_contract():
    """lc_pnp_ransac_workspace_bytes: B arrival counters (padded to 16 bytes), (B, H, 12) doubles + floats for the hypotheses and
    (B, chunks of 64 points, H) count/error partials, H = iterations rounded up to 64; a smaller workspace is refused before anything
    is launched (no GPU needed), by both split-form entry points."""
    from lc_amd import _lib

    lib = _lib.load()
    assert lib.lc_pnp_ransac_workspace_bytes(0, 10, 150) == 0 and lib.lc_pnp_ransac_workspace_bytes(4, 10, 0) == 0
    B, N, H = 5, 1000, 192
    chunks = (N + 63) // 64
    ctr = 16 * ((B + 3) // 4)  # the doubles behind the counters are read as 16-byte pairs
    assert lib.lc_pnp_ransac_workspace_bytes(B, N, 150) == ctr + B * H * 12 * (8 + 4) + B * chunks * H * 8
    assert lib.lc_pnp_ransac_workspace_bytes(B, 16384, 150) == ctr + B * H * 12 * 12 + B * 256 * H * 8  # every point of a row is scored
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    rc = lib.lc_pnp_ransac_init5_f32(p, p, p, None, B, N, 2.0, None, 150, 0, p, p, p, p, None, None, p, 64, 0, None, None, 4, 0, None, None,
                                     None, None, None, 0, None)
    assert rc != 0 and b"workspace" in lib.lc_amd_last_error()
    rc = lib.lc_pnp_ransac_init5_f32(p, p, p, None, B, N, 2.0, None, 150, 0, p, p, p, p, None, None, None, 0, 0, p, None, 4, 0, p, p, p, None,
                                     None, 0, None)  # selection asked for, no counts output
    assert rc != 0 and b"selection" in lib.lc_amd_last_error()
    # the section offsets the diagnostics read the workspace through come from the library (lc_pnp_init.hip: carve_workspace)
    lay = (ctypes.c_size_t * 6)()
    assert lib.lc_pnp_ransac_workspace_layout(B, N, 150, lay) == 0
    assert list(lay) == [ctr, ctr + B * H * 12 * 8, ctr + B * H * 12 * 12, H, chunks, lib.lc_pnp_ransac_workspace_bytes(B, N, 150)]
    assert lib.lc_pnp_ransac_workspace_layout(0, N, 150, lay) != 0


def test_extended_entry_points_reject_bad_arguments_before_launching():
    """lc_pnp_lm3_f32 / lc_dense_frontend_fwd3: argument errors are reported by return code + lc_amd_last_error, nothing is
    launched (runs without a GPU)."""
    from lc_amd import _lib

    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    err = lambda: lib.lc_amd_last_error().decode()
    # two weight forms at once / none at all
    assert lib.lc_pnp_lm3_f32(p, p, p, p, p, None, None, p, p + 64, p, p, None, 2, 4, 5, 1e-6, 0, 0, None, 0, None) != 0 and "exactly one" in err()
    assert lib.lc_pnp_lm3_f32(p, p, p, None, None, None, None, p, p + 64, p, p, None, 2, 4, 5, 1e-6, 0, 0, None, 0, None) != 0 and "exactly one" in err()
    # unknown option bit, icov flag without the diagonal weights, shared poses without a separate start
    assert lib.lc_pnp_lm3_f32(p, p, p, None, p, None, None, p, p + 64, p, p, None, 2, 4, 5, 1e-6, 8, 0, None, 0, None) != 0 and "option" in err()
    assert lib.lc_pnp_lm3_f32(p, p, p, None, None, p, None, p, p + 64, p, p, None, 2, 4, 5, 1e-6, 1, 0, None, 0, None) != 0 and "weights_diag" in err()
    assert lib.lc_pnp_lm3_f32(p, p, p, None, p, None, None, None, p + 64, p, p, None, 2, 4, 5, 1e-6, 0, 1, None, 0, None) != 0 and "start" in err()
    # visibility logits without a mask buffer
    assert lib.lc_dense_frontend_fwd3(p, p, p, None, p, 0.5, 0, 0, 0, 0, 0, 0, 1, 4, 4, 0, 0, 2, p, p, p, p, None, None) != 0 and "vis_" in err()
    # empty batches are fine
    assert lib.lc_pnp_lm3_f32(p, p, p, None, p, None, None, p, p + 64, p, p, None, 0, 4, 5, 1e-6, 0, 0, None, 0, None) == 0


def test_product_path_has_no_cpu_fallback():
    from lc_amd import synth
    from lc_amd.cov_mixed import Loss_cov_mixed
    from lc_amd.pnp import cer_solver
    from lc_amd.ptnet import softargmax_2d_std

    b = synth.make_batch(2, 8, seed=0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        Loss_cov_mixed(b["K"], b["pose"], b["pts3d"], b["pts2d"], b["inv_std"], None, bbox_3d=b["bbox_3d"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        softargmax_2d_std(torch.rand(2, 3, 8, 8))
    with pytest.raises(TypeError):
        from lc_amd import _lib
        _lib.require_hip_f32("x", [1, 2, 3])


def test_ragged_jobs_become_one_padded_batch():
    from lc_amd.pnp.cer_solver import _batch_tensors

    a = [torch.ones(3, 2), torch.ones(5, 2) * 2, torch.ones(1, 2) * 3]
    (bt, cnt, none, same) = _batch_tensors(a, [3, 5, 1], None, [torch.zeros(7), torch.ones(7), torch.zeros(7)])
    assert bt.shape == (3, 5, 2) and none is None and cnt.tolist() == [3, 5, 1] and same.shape == (3, 7)
    assert bt[0, 3:].abs().sum() == 0 and bt[2, 1:].abs().sum() == 0 and (bt[1] == 2).all()
    already = torch.rand(3, 4, 2)
    assert _batch_tensors(already)[0] is already or torch.equal(_batch_tensors(already)[0], already)


def test_cer_solver_surface_on_oracle_backend(oracle_backend):
    """Ragged lists + NaN filtering + invalid -> start + optimal_start, with the LM solve supplied by the oracle."""
    from lc_amd import synth
    from lc_amd.pnp import cer_solver

    b = synth.make_batch(5, 24, seed=3)
    n = [24, 10, 2, 24, 7]
    pts3d = [b["pts3d"][i, :n[i]] for i in range(5)]
    pts2d = [b["pts2d"][i, :n[i]].clone() for i in range(5)]
    pts2d[1][0, 1] = float("nan")
    icov = [b["inv_std"][i, :n[i]] ** 2 for i in range(5)]
    inv, st = cer_solver.solve(b["K"], pts3d, pts2d, icov, list(b["start"]), num_workers=4, filter_input_nan=True)
    assert st.shape == (5, 7) and inv["invalids"].tolist()[2] is True
    assert torch.equal(st[2], b["start"][2])
    ok = ~inv["invalids"]
    assert (st[ok] - b["start"][ok]).abs().max() > 1e-3  # moved away from the start
    inv2, st2 = cer_solver.solve(b["K"], b["pts3d"], b["pts2d"], b["inv_std"] ** 2, b["start"], optimal_start=True)
    assert torch.equal(st2, b["start"]) and not inv2["invalids"].any()


@pytest.mark.parametrize("kind", ["sparse", "dense", "bin"])
def test_loss_fn_matches_reference_trajectory(oracle_backend, kind):
    """lc_amd.losses.Loss_fn (host logic) + oracle loss == the reference's Loss_fn over the warm-up ramp, incl. the
    NormClipper.max_norm buffer trajectory and the gradients on the network outputs."""
    from lc_amd.losses import Loss_fn
    from tests.golden.gen_golden_lossfn import run

    z = np.load(os.path.join(GOLDEN, f"lossfn_{kind}_f64.npz"))
    rec = run(Loss_fn, kind, list(z["steps"]), torch.float64)
    assert set(rec) == set(z.files)
    for k in z.files:
        if k == "steps":
            continue
        # losses/state to 1e-8; gradients pass through the EMA-clipped hooks, where 1e-10 oracle-vs-reference
        # differences of tiny LC gradients are amplified relative to the tensor max -> 1e-6.  The dense gradients also
        # follow MKL's code path: off its AVX-512 kernels (MKL_ENABLE_INSTRUCTIONS=SSE4_2, the path it takes on AMD
        # CPUs) they move by up to 5e-6 against the goldens -> 1e-5 for those
        grad_tol = 1e-5 if kind == "dense" else 1e-6
        assert rel_err(rec[k], z[k]) <= (grad_tol if "_grad_" in k else 1e-8), k
    z32 = np.load(os.path.join(GOLDEN, f"lossfn_{kind}_f32.npz"))
    rec32 = run(Loss_fn, kind, list(z32["steps"]), torch.float32)
    for k in z32.files:
        if re.match(r"s\d+_w?loss_", k):
            assert abs(float(rec32[k]) - float(z32[k])) <= 1e-4 * max(1.0, abs(float(z32[k]))), k


@pytest.mark.parametrize("kind", ["dense_glmo", "bin_zlmo", "sparse_metric", "dense_plumb"])
def test_loss_fn_matches_reference_at_training_shapes(oracle_backend, kind):
    """The same host logic + oracle at the reference's own training shapes (configs/glmo.yaml: 64x64 maps, stride 2, N=1024;
    configs/zlmo.yaml: 128x128 maps, stride 3, N=1849, 21 code planes; gsplmo's loss block at B=256 N=64; BASELINE configs[0]'s plumbing
    case: 16 crops, 32x32 maps, stride 2, N=256) against the trajectories the
    unmodified reference class produced (tests/golden/gen_golden_lossfn.py --train-shapes): float64 losses / states to 1e-8, gradients
    (stored rounded to float32) to 1e-6 of their largest entry; the float32 run against the reference's float32 scalars to 1e-4."""
    from lc_amd.losses import Loss_fn
    from tests.golden.gen_golden_lossfn import TRAIN_KINDS, run

    z = np.load(os.path.join(GOLDEN, f"lossfn_{kind}.npz"))
    assert list(z["steps"]) == TRAIN_KINDS[kind][0]
    rec = run(Loss_fn, kind, list(z["steps"]), torch.float64)
    assert set(rec) == {k for k in z.files if not k.startswith("f32_")}
    for k in rec:
        if k != "steps":
            assert rel_err(rec[k], z[k]) <= (1e-6 if "_grad_" in k else 1e-8), k
    rec32 = run(Loss_fn, kind, list(z["steps"]), torch.float32)
    for k in z.files:
        if re.match(r"f32_s\d+_w?loss_", k):
            assert abs(float(rec32[k[4:]]) - float(z[k])) <= 1e-4 * max(1.0, abs(float(z[k]))), k
        elif k.startswith("f32_") and "_state_" in k:
            assert rel_err(rec32[k[4:]], z[k]) <= 1e-3, k


def test_loss_fn_state_dict_keys_match_reference_checkpoints():
    from lc_amd.config import AttrDict
    from lc_amd.losses import Loss_fn

    fn = Loss_fn(AttrDict(pose_loss_cfg=dict(type="cov", clip_weight_grad=True)), AttrDict())
    assert list(fn.state_dict().keys()) == ["weight_grad_clipper.max_norm"]
    fn2 = Loss_fn(AttrDict(pose_loss_cfg=dict(clip_weight_grad=True, clip_scale_grad=True, clip_pts_grad=True)), AttrDict())
    assert set(fn2.state_dict()) == {"weight_grad_clipper.max_norm", "scale_grad_clipper.max_norm", "pts_grad_clipper.max_norm"}
    fn3 = Loss_fn(AttrDict(pose_loss_cfg=dict()), AttrDict(), total_bit_cnt=16)
    assert set(fn3.state_dict()) == {"weight_grad_clipper.max_norm", "xyz_bin_loss_fn.histogram"}  # losses.py:199


def test_dense_matching_shapes_and_phase():
    from lc_amd.losses import dense_pnp_matching_from_xyz

    xyz, w = torch.randn(2, 3, 9, 10), torch.rand(2, 2, 9, 10)
    msk = torch.rand(2, 9, 10) > 0.5
    p2, s, p3, v = dense_pnp_matching_from_xyz(xyz, w, msk, torch.tensor([[1.0, 2, 3], [4, 5, 6]]), sample=3, top_left=(1, 2))
    assert p2.shape == (2, 9, 2) and s.shape == (2, 9, 2) and p3.shape == (2, 9, 3) and v.shape == (2, 9)
    assert p2[0, 0].tolist() == [2.0, 1.0]  # (x, y) of the first sampled pixel
    assert torch.allclose(p3[1, 0], xyz[1, :, 1, 2] * torch.tensor([4.0, 5, 6]))
    assert torch.equal(s[0, 4], w[0, :, 4, 5])


# A stand-in checkout with the module layout and the names the drop-in installer rebinds (lc_amd/dropin.py): each module defines its own
# placeholder objects, so that every rebinding is visible as an identity change.
_STAND_IN_CHECKOUT = {
    "lib/cov_mixed.py": "class Loss_cov_mixed:\n    pass\n",
    "lib/pnp/pnp_ceres.py": "def solve(*a, **k):\n    raise RuntimeError('the Ceres extension of the checkout')\n",
    "lib/pnp/cer_solver.py": "from lib.pnp import pnp_ceres\n",
    "lib/pnp/cv2_solver.py": "import cv2\n",
    "lib/utils/grad.py": "import torch\n\n\nclass NormClipper(torch.nn.Module):\n    pass\n",
    "losses.py": ("import torch\nfrom lib.cov_mixed import Loss_cov_mixed\nfrom lib.utils.grad import NormClipper\n\n\n"
                  "class Loss_fn(torch.nn.Module):\n"
                  "    def __init__(self, cfg, cfg_global, total_bits=0):\n"
                  "        super().__init__()\n"
                  "        pose = cfg.pose_loss_cfg\n"
                  "        self.weight_grad_clipper = NormClipper() if pose.get('clip_weight_grad', True) else None\n"
                  "        self.scale_grad_clipper = NormClipper(rel_thresh=2) if pose.get('clip_scale_grad', False) else None\n\n"
                  "    def sparse_kpt_loss(self, *a):\n        raise NotImplementedError\n\n"
                  "    def dense_pose_loss(self, *a):\n        raise NotImplementedError\n"),
    "ptnet.py": ("import torch\n\n\ndef softargmax_2d_std(x):\n    raise NotImplementedError\n\n\n"
                 "class ptnet(torch.nn.Module):\n    def forward(self, rgb):\n        raise NotImplementedError\n"),
}


def test_dropin_install_rebinds_the_entry_points_of_a_stand_in_checkout(tmp_path):
    import subprocess
    import sys

    for rel, text in _STAND_IN_CHECKOUT.items():
        os.makedirs(os.path.dirname(os.path.join(tmp_path, rel)), exist_ok=True)
        with open(os.path.join(tmp_path, rel), "w") as f:
            f.write(text)
    code = (
        "import sys, warnings; warnings.filterwarnings('ignore'); sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
        "import lc_amd.dropin as d; r = d.install(); print(r)\n"
        "import lib.cov_mixed, losses, ptnet, lc_amd.cov_mixed as cm, lc_amd.ptnet as hp\n"
        "from lib.pnp import cer_solver, pnp_ceres\n"
        "assert lib.cov_mixed.Loss_cov_mixed is cm.Loss_cov_mixed and losses.Loss_cov_mixed is cm.Loss_cov_mixed\n"
        "assert cer_solver.__name__ == 'lc_amd.pnp.cer_solver' and pnp_ceres.__name__ == 'lc_amd.pnp.pnp_ceres'\n"
        "from lib.pnp import cv2_solver; assert cv2_solver.__name__ == 'lc_amd.pnp.gpu_solver'  # no OpenCV in this image\n"
        "assert ptnet.softargmax_2d_std is hp.softargmax_2d_std and ptnet.ptnet.forward.__module__ == 'lc_amd.dropin'\n"
        "import lc_amd.grad as g, lc_amd.losses as ol, lib.utils.grad as rg\n"
        "assert rg.NormClipper is g.NormClipper and losses.NormClipper is g.NormClipper\n"
        "assert losses.Loss_fn.dense_pose_loss is ol.Loss_fn.dense_pose_loss and losses.Loss_fn.sparse_kpt_loss is ol.Loss_fn.sparse_kpt_loss\n"
        "from lc_amd.config import AttrDict\n"
        "fn = losses.Loss_fn(AttrDict(pose_loss_cfg=dict(type='cov', clip_weight_grad=True, clip_scale_grad=True), seg_loss_type='L1'), AttrDict())\n"
        "assert type(fn.weight_grad_clipper) is g.NormClipper and set(fn.state_dict()) == {'weight_grad_clipper.max_norm', 'scale_grad_clipper.max_norm'}\n"
        "assert all(r.values()), r\n" % (str(tmp_path), ROOT))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]


def test_xyz_to_nn_target_inverts_nn_out_to_xyz_for_the_continuous_head():
    from lc_amd.losses import nn_out_to_xyz, xyz_to_nn_target

    g = torch.Generator().manual_seed(0)
    xyz = torch.randn(2, 5, 6, 3, generator=g) * 30
    scale = torch.tensor([[37.8, 37.9, 45.8], [10.0, 20.0, 30.0]])
    tgt, raw = xyz_to_nn_target(xyz, scale)
    assert raw is None and tgt.shape == (2, 3, 5, 6)
    assert torch.allclose(nn_out_to_xyz(tgt, scale), xyz, atol=1e-5)


def test_rt_to_quaternion_rep_round_trips_all_branches():
    """Every branch of the component selection (w, x, y or z largest, incl. 180-degree turns) round-trips through quaternion_rep_to_RT."""
    from lc_amd.transforms import RT_to_quaternion_rep, quaternion_rep_to_RT

    g = torch.Generator().manual_seed(0)
    q = torch.randn(200, 4, generator=g, dtype=torch.float64)
    q[:4] = torch.eye(4, dtype=torch.float64)          # identity and the three half turns
    q[4:8] = torch.eye(4, dtype=torch.float64) + 1e-9  # next to them
    q = q / q.norm(dim=-1, keepdim=True)
    t = torch.randn(200, 3, generator=g, dtype=torch.float64)
    R, _ = quaternion_rep_to_RT(torch.cat((q, t), -1))
    rep = RT_to_quaternion_rep(R, t)
    assert rep.shape == (200, 7) and torch.allclose(rep[:, :4].norm(dim=-1), torch.ones(200, dtype=torch.float64), atol=1e-12)
    sgn = torch.sign((rep[:, :4] * q).sum(-1, keepdim=True))
    assert (rep[:, :4] * sgn - q).abs().max() < 1e-7 and torch.equal(rep[:, 4:], t)
    k = rep[:, :4].abs().argmax(-1)
    assert (rep[torch.arange(200), k] > 0).all() and set(k.tolist()) == {0, 1, 2, 3}
    R2, _ = quaternion_rep_to_RT(rep)
    assert (R2 - R).abs().max() < 1e-12


# A stand-in for the reference's `losses` module: the label-preparation names, written here from the formulas the tests state (the
# projection of homogeneous depth back to object coordinates; the best candidate pose = the only one), each recording its call.
_STAND_IN_LOSSES = """
import torch

CALLS = []


def xyz_from_homo_z(homo_z, R, t, K):
    CALLS.append("xyz_from_homo_z")
    return homo_z @ (torch.linalg.inv(K).unsqueeze(-3).mT @ R.unsqueeze(-3)) - (t[:, None, None, :] @ R.unsqueeze(-3))


def selete_best_pose(gt_dict, out_dict, sym_aware_started):
    CALLS.append("selete_best_pose")
    Rt = gt_dict["Rt_candi"][0][:, 0]
    pose = torch.cat((torch.zeros(len(Rt), 4), Rt[..., 3]), -1)
    return Rt, pose, xyz_from_homo_z(gt_dict["homo_z_out"], gt_dict["R_no_aug"], gt_dict["t_no_aug"], gt_dict["K_no_aug"])


def annots_on_the_fly(gt_dict, out_dict, cfg_global, step):
    CALLS.append("annots_on_the_fly")
    return gt_dict, out_dict, cfg_global, step
"""


def test_label_prep_names_pass_through_to_the_reference(monkeypatch, tmp_path):
    """`lc_amd.losses.annots_on_the_fly / selete_best_pose / xyz_from_homo_z` (label preparation, outside the hot path) delegate to
    the reference's own module when a checkout is reachable, and raise ImportError otherwise.  The checkout
    is a stand-in written to tmp_path: what is checked is the pass-through (arguments in, the module's results out)."""
    import os
    import sys

    import lc_amd.losses as L

    monkeypatch.delenv("LC_REFERENCE", raising=False)
    monkeypatch.delitem(sys.modules, "losses", raising=False)
    with pytest.raises(ImportError):
        L.xyz_from_homo_z(None, None, None, None)
    ref = str(tmp_path)
    with open(os.path.join(ref, "losses.py"), "w") as f:
        f.write(_STAND_IN_LOSSES)
    monkeypatch.setenv("LC_REFERENCE", ref)
    monkeypatch.setattr(sys, "path", list(sys.path))
    g = torch.Generator().manual_seed(0)
    B, H, W = 2, 4, 5
    homo_z = torch.randn(B, H, W, 3, generator=g)
    R = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))[0]
    t, K = torch.randn(B, 3, generator=g), torch.eye(3).expand(B, 3, 3) + 0.1 * torch.randn(B, 3, 3, generator=g)
    got = L.xyz_from_homo_z(homo_z, R, t, K)
    want = homo_z @ (torch.linalg.inv(K).unsqueeze(-3).mT @ R.unsqueeze(-3)) - (t[:, None, None, :] @ R.unsqueeze(-3))
    assert torch.allclose(got, want, atol=1e-5)
    gt = dict(Rt_candi=[torch.cat((R, t[..., None]), -1).unsqueeze(-3)], homo_z_out=homo_z, R_no_aug=R, t_no_aug=t, K_no_aug=K,
              msk_noc=torch.ones(B, H, W))
    Rt_best, pose_best, xyz_gt = L.selete_best_pose(gt, {}, False)
    assert Rt_best.shape == (B, 3, 4) and pose_best.shape == (B, 7) and torch.allclose(xyz_gt, want, atol=1e-5)
    cfg = object()
    assert L.annots_on_the_fly(gt, {}, cfg, 7) == (gt, {}, cfg, 7)
    ref_mod = sys.modules["losses"]
    assert os.path.dirname(os.path.abspath(ref_mod.__file__)) == os.path.abspath(ref)
    assert ref_mod.CALLS == ["xyz_from_homo_z", "selete_best_pose", "xyz_from_homo_z", "annots_on_the_fly"]


def test_chain_and_round3_entry_points_check_their_arguments_before_launching():
    """lc_pnp_lm_chain2_f32 (plain C struct jobs), lc_dense_frontend_select3, lc_dense_aux_fwd2, lc_xyz_bin_loss_fwd2 / _counts / _finish: argument
    errors come back as return code + lc_amd_last_error and empty batches are no-ops, all without touching a GPU."""
    from lc_amd import _lib
    from lc_amd.pnp.pnp_ceres import _Job

    lib = _lib.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.addressof(buf)
    empty = _Job(None, None, None, None, None, None, None, None, None, None, None, None, 0, 700, 20, 1e-6, 0, 0)
    assert lib.lc_pnp_lm_chain2_f32(ctypes.byref(empty), ctypes.byref(empty), None, 0, None) == 0  # two empty batches
    assert lib.lc_pnp_lm_chain2_f32(None, ctypes.byref(empty), None, 0, None) != 0 and b"null job" in lib.lc_amd_last_error()
    bad = _Job(p, p, p, None, p, None, None, None, p, p, p, None, 4, 700, 20, 1e-6, 8, 0)  # unknown option bit
    assert lib.lc_pnp_lm_chain2_f32(ctypes.byref(empty), ctypes.byref(bad), None, 0, None) != 0 and b"option" in lib.lc_amd_last_error()
    two = _Job(p, p, p, p, p, None, None, None, p, p, p, None, 4, 700, 20, 1e-6, 0, 0)  # two weight forms at once
    assert lib.lc_pnp_lm_chain2_f32(ctypes.byref(two), ctypes.byref(empty), None, 0, None) != 0 and b"exactly one" in lib.lc_amd_last_error()
    # front end + selection: more sampled pixels than the one launch takes; a mask mode without visibility logits
    rc = lib.lc_dense_frontend_select3(p, p, p, None, p, 0.5, 0, 0, 0, 0, 0, 0, 1, 258, 256, 0, 0, 2, 0, 0.5, 1, 4, 0, 0, p, p, p, None, p, None, 0, None)
    assert rc != 0 and b"16384" in lib.lc_amd_last_error()
    rc = lib.lc_dense_frontend_select3(p, p, p, None, None, 0.5, 0, 0, 0, 0, 0, 0, 1, 64, 64, 0, 0, 2, 2, 0.5, 1, 4, 0, 0, p, p, p, None, p, None, 0, None)
    assert rc != 0 and b"visibility" in lib.lc_amd_last_error()
    assert lib.lc_dense_frontend_select3(p, p, p, None, p, 0.5, 0, 0, 0, 0, 0, 0, 0, 64, 64, 0, 0, 2, 0, 0.5, 1, 4, 0, 0, p, p, p, None, p, None, 0, None) == 0
    # dense auxiliary losses: xyz without exactly one mask form; unknown loss type; empty batch
    rc = lib.lc_dense_aux_fwd2(p, None, None, p, p, p, None, 0, 0, 0, 0, 2, 64, 0, p, p, p, None)
    assert rc != 0 and b"mask" in lib.lc_amd_last_error()
    assert lib.lc_dense_aux_fwd2(None, None, None, None, p, p, None, 0, 0, 0, 0, 2, 64, 7, p, p, p, None) != 0
    assert lib.lc_dense_aux_fwd2(None, None, None, None, p, p, None, 0, 0, 0, 0, 0, 64, 0, p, p, p, None) == 0
    # code loss: more bits than the kernel's per-bit tables hold
    rc = lib.lc_xyz_bin_loss_fwd2(p, p, p, 0, 0, 0, 2, 200, 64, 0.05, p, p, p, p, p, None)
    assert rc != 0 and b"128" in lib.lc_amd_last_error()
    assert lib.lc_xyz_bin_loss_fwd2(p, p, p, 0, 0, 0, 0, 17, 64, 0.05, p, p, p, p, p, None) == 0
    # its sharded form: counts without the place for the BCE means; a finish without counts; an empty batch
    assert lib.lc_xyz_bin_loss_counts(p, p, p, 0, 0, 0, 2, 17, 64, p, None, p, p, None) != 0 and b"null" in lib.lc_amd_last_error()
    assert lib.lc_xyz_bin_loss_counts(p, p, p, 0, 0, 0, 2, 17, 64, None, p, p, p, None) != 0
    assert lib.lc_xyz_bin_loss_counts(p, p, p, 0, 0, 0, 0, 17, 64, p, p, p, p, None) == 0
    assert lib.lc_xyz_bin_loss_finish(None, p, 17, 0.05, p, p, p, None) != 0 and b"null" in lib.lc_amd_last_error()
    assert lib.lc_xyz_bin_loss_finish(p, p, 200, 0.05, p, p, p, None) != 0 and b"128" in lib.lc_amd_last_error()


def test_training_shape_fixtures_span_the_warm_up_ramp_and_the_reference_shapes():
    """What VERDICT r4 #1 asked the new fixtures to be: the reference's own shapes and loss blocks, steps across the warm-up ramp (losses.py:272-276,
    296-302), at least three consecutive calls for the clipper's trajectory -- checked on the committed files and the seeded inputs."""
    from lc_amd import synth
    from lc_amd.config import AttrDict
    from lc_amd.losses import pose_loss_factor
    from tests.golden.gen_golden_lossfn import TRAIN_KINDS

    shapes = {"dense_glmo": ((4, 3, 64, 64), 2, 1024), "bin_zlmo": ((4, 21, 128, 128), 3, 1849), "dense_plumb": ((16, 3, 32, 32), 2, 256)}
    for kind, (steps, spe, bits) in TRAIN_KINDS.items():
        cfg = AttrDict(synth.TRAIN_LOSS_CONFIGS[kind])
        f = [pose_loss_factor(cfg, s, spe) for s in steps]
        assert len(steps) >= 3 and min(f) < 1e-3 and any(0.4 < v < 0.6 for v in f) and max(f) == 1.0, (kind, f)
        gt, out = synth.train_inputs(kind, seed=0)
        gt2, out2 = synth.train_inputs(kind, seed=0)
        assert all(torch.equal(out[k], out2[k]) for k in out)  # seeded
        z = np.load(os.path.join(GOLDEN, f"lossfn_{kind}.npz"))
        if kind in shapes:
            shape, stride, n = shapes[kind]
            head = "xyz_noc_bin" if bits else "xyz_noc"
            assert tuple(out[head].shape) == shape and z[f"s0_grad_{head}"].shape == shape and z[f"s0_grad_{head}"].dtype == np.float32
            H = shape[-1]
            assert (-(-H // stride)) ** 2 == n and cfg["pose_loss_cfg"].get("dense_sample", 2) == stride
            assert sum(gt.get("bit_cnt", [])) == bits
            assert 0.1 < float(gt["msk_vis"].mean()) < 0.5 and float(gt["msk_vis"].sum()) < float(gt["msk_noc"].sum())  # an object with an occluded part
            mn = [float(z[f"s{i}_state_weight_grad_clipper.max_norm"]) for i in range(len(steps))]
            assert len(set(mn)) == len(mn) and min(mn) > 0
        else:
            assert tuple(out["pts2d"].shape) == (256, 64, 2) and z["s0_grad_pts2d"].shape == (256, 64, 2)


@pytest.mark.parametrize("name", ["main", "optim", "posecov", "render", "crop", "models", "symerr", "vsd", "gtinfo", "maskcrop", "augment", "rle", "geometry"])
def test_shared_loader_refuses_what_it_cannot_rebuild(name, tmp_path, monkeypatch):
    """The refusal branches of the one loader behind every module's load(), without a compiler run and without a dlopen: a library built
    from other sources on a box without hipcc, and a missing library where building is not wanted.  Every target of the registry: the
    messages name the paths and the hashes of the target they were given."""
    from lc_amd import _lib, build

    assert [t.name for t in build.TARGETS].count(name) == 1
    target = next(t for t in build.TARGETS if t.name == name)._replace(so_path=str(tmp_path / f"lib_{name}.so"))
    monkeypatch.setattr(build, "hipcc_available", lambda: False)
    monkeypatch.setattr(build, "build", lambda *a, **k: pytest.fail("the loader must not try to build here"))
    monkeypatch.delenv("LC_AMD_ALLOW_STALE", raising=False)
    with pytest.raises(RuntimeError) as e:  # missing, and the caller does not want a build
        _lib.load_target(target, {}, build_if_missing=False)
    assert str(e.value) == f"lc_amd: {target.so_path} is missing or stale; run `python __graft_entry__.py build`"
    open(target.so_path, "wb").write(b"\x7fELF no marker in here")
    for build_if_missing in (True, False):  # there, built from other sources (no hash inside), and no compiler to rebuild it with
        with pytest.raises(RuntimeError) as e:
            _lib.load_target(target, {}, build_if_missing=build_if_missing)
        msg = str(e.value)
        assert msg.startswith(f"lc_amd: {target.so_path} was built from other sources than the ones next to it (embedded hash None, "
                              f"sources {build.source_hash(target)}) and hipcc is not available")
        assert msg.endswith("set LC_AMD_ALLOW_STALE=1 to load it as it is")
    others = {build.source_hash(t) for t in build.TARGETS if t.name != name}
    assert len(others) == len(build.TARGETS) - 1 and not any(h in msg for h in others)


def test_every_build_switch_is_listed_in_the_design():
    """The names the kernels' sources test with #ifdef / #ifndef (the per-library source-hash macros apart) are exactly the rows of
    DESIGN.md's table of build switches: a new switch cannot appear without an entry that says who sets it, and a folded one leaves
    the table with its code."""
    import glob

    in_sources = set()
    for path in glob.glob(os.path.join(ROOT, "lc_amd", "csrc", "**", "*"), recursive=True):
        if os.path.isfile(path):
            in_sources |= set(re.findall(r"^\s*#\s*ifn?def\s+(LC_\w+)", open(path).read(), re.M))
    in_sources = {n for n in in_sources if not re.fullmatch(r"LC_AMD_\w*SRC_HASH", n)}
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    table = design[design.index("## 9. Build switches"):]
    listed = set(re.findall(r"^\| `(LC_\w+)` \|", table, re.M))
    assert len(in_sources) >= 10 and in_sources == listed, (sorted(in_sources - listed), sorted(listed - in_sources))


def test_upper_rank_classifier_tells_duplicate_near_and_far_apart():
    """The host-side classifier behind tests/test_gpu_select.py's coverage condition, on hand-made key lists: rank 1.5 of four keys lies
    between keys[1] and keys[2]."""
    from tests.test_gpu_select import quantile_in_mask_q, upper_rank_class, weight_keys

    k = 0xBF800000
    assert upper_rank_class(np.array([k - 9, k, k, k + 0x300], dtype=np.uint32), 0.5) == "duplicate"
    assert upper_rank_class(np.array([k - 9, k, k + 0xFF, k + 0x300], dtype=np.uint32), 0.5) == "near"  # same upper 24 bits
    assert upper_rank_class(np.array([k - 9, k + 0xFF, k + 0x100, k + 0x300], dtype=np.uint32), 0.5) == "far"  # one apart, across the prefix
    assert upper_rank_class(np.array([k, k, k + 1, k + 1, k + 2], dtype=np.uint32), 0.5) == "integral"  # rank 2.0
    assert upper_rank_class(np.array([k, k + 1], dtype=np.uint32), 1.5) == "integral"  # q clamped to 1: rank n - 1
    # the keys ascend with the weights (negative ones below zero below positive ones) and the mode-2 quantile is the kernels' fp32 value
    w = np.array([-2.0, -0.0, 0.0, 1e-30, 0.5, 0.5000001, 3.0], dtype=np.float32)
    keys = weight_keys(w)
    assert keys.dtype == np.uint32 and np.all(np.diff(keys.astype(np.int64)) > 0)
    assert quantile_in_mask_q(0.2, 1024, 4096) == np.float32(0.8) and quantile_in_mask_q(0.2, 0, 7) == np.float32(1.0)
