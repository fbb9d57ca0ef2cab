"""GPU parity of the fused spatial-softmax + soft-argmax kernels against golden vectors from ptnet.py (fp32 and fp64)."""
import numpy as np
import pytest
import torch

from tests import rowwise as rw
from tests.util import golden_files, case_name, rel_err

pytestmark = pytest.mark.gpu
FILES = golden_files("head_")


@pytest.mark.parametrize("path", FILES, ids=[case_name(p, "head_") for p in FILES])
def test_head_vs_golden(path):
    from lc_amd.ptnet import spatial_softargmax_2d_std, softargmax_2d_std

    z = np.load(path)
    dev = torch.device("cuda:0")
    lg = torch.from_numpy(z["in_logits"]).to(dev).requires_grad_(True)
    ctm, cts = torch.from_numpy(z["in_ct_mean"]).to(dev), torch.from_numpy(z["in_ct_std"]).to(dev)
    mean, std = spatial_softargmax_2d_std(lg)
    (gl,) = torch.autograd.grad([mean, std], [lg], [ctm, cts])
    # pixel-unit outputs in [0, 63]: 2e-4 px abs (fp32 reference itself sits ~1e-5 from fp64)
    assert (mean.detach().cpu().double() - torch.from_numpy(z["f64_mean"])).abs().max().item() <= 2e-4
    assert (std.detach().cpu().double() - torch.from_numpy(z["f64_std"])).abs().max().item() <= 2e-4
    assert rel_err(gl.cpu(), z["f64_g_logits"]) <= 2e-4
    assert rel_err(gl.cpu(), z["f32_g_logits"]) <= 2e-4
    # map by map (tests/rowwise.py): the same 2e-4 against each map's own largest gradient entry, the reference's fp32 run setting the bound
    # where it exceeds that on a map
    maps = (-1,) + tuple(lg.shape[-2:])
    rw.check_kept("head g_logits per map", gl, z["f64_g_logits"], z["f32_g_logits"], 2e-4, rows=maps)
    # the function on its own (probabilities in), ptnet.py:100-115
    pr = torch.from_numpy(z["f32_prob"]).to(dev).requires_grad_(True)
    m2, s2 = softargmax_2d_std(pr)
    (gp,) = torch.autograd.grad([m2, s2], [pr], [ctm, cts])
    assert (m2.detach().cpu().double() - torch.from_numpy(z["f64_mean"])).abs().max().item() <= 2e-4
    assert (s2.detach().cpu().double() - torch.from_numpy(z["f64_std"])).abs().max().item() <= 2e-4
    assert rel_err(gp.cpu(), z["f32_g_prob"]) <= 2e-4


@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (2, 2, 128, 128), (1, 1, 16, 20), (2, 3, 30, 50)])
def test_head_odd_shapes_vs_torch(shape):
    """Non-power-of-two / non-multiple-of-4 maps (scalar path) and the 128x128 zlmo size, vs a float64 torch restatement."""
    from lc_amd.ptnet import spatial_softargmax_2d_std
    from oracle.softargmax_oracle import spatial_softargmax_2d_std as orc

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    lg = (torch.randn(shape, generator=g) * 3)
    ctm, cts = torch.randn(shape[:2] + (2,), generator=g), torch.randn(shape[:2] + (2,), generator=g)
    x = lg.to(dev).requires_grad_(True)
    mean, std = spatial_softargmax_2d_std(x)
    (gl,) = torch.autograd.grad([mean, std], [x], [ctm.to(dev), cts.to(dev)])
    x64 = lg.double().requires_grad_(True)
    m64, s64 = orc(x64)
    (g64,) = torch.autograd.grad([m64, s64], [x64], [ctm.double(), cts.double()])
    assert (mean.detach().cpu().double() - m64.detach()).abs().max().item() <= 3e-4
    assert (std.detach().cpu().double() - s64.detach()).abs().max().item() <= 3e-4
    assert rel_err(gl.cpu(), g64) <= 3e-4
    x32 = lg.clone().requires_grad_(True)
    (g32,) = torch.autograd.grad(orc(x32), [x32], [ctm, cts])
    rw.check_kept(f"head {shape} g_logits per map", gl, g64, g32, 3e-4, rows=(-1,) + shape[-2:])


def test_head_full_size_properties():
    """BASELINE head size (256,64,64,64): probabilities sum to one => sum of the logit-gradient over each map is ~0;
    a one-hot-ish map returns its peak location; shifting the logits by a constant changes nothing."""
    from lc_amd.ptnet import spatial_softargmax_2d_std
    from lc_amd import synth

    dev = torch.device("cuda:0")
    lg = synth.make_head_logits(256, 64, 64, 64, seed=3).to(dev).requires_grad_(True)
    mean, std = spatial_softargmax_2d_std(lg)
    (g,) = torch.autograd.grad([mean.sum() + std.sum()], [lg])
    assert g.flatten(-2).sum(-1).abs().max().item() <= 1e-3
    m2, s2 = spatial_softargmax_2d_std(lg.detach() + 7.5)
    assert (m2 - mean).abs().max().item() <= 1e-4 and (s2 - std).abs().max().item() <= 1e-4
    spike = torch.full((4, 1, 64, 64), -30.0, device=dev)
    spike[:, :, 17, 42] = 30.0
    m3, s3 = spatial_softargmax_2d_std(spike)
    assert torch.allclose(m3, torch.tensor([42.0, 17.0], device=dev).expand(4, 1, 2), atol=1e-4)
    assert (s3 - 1e-3).abs().max().item() <= 1e-4  # sqrt(0 + 1e-6)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("shape", [(3, 5, 64, 64), (2, 3, 128, 128), (2, 2, 24, 40), (2, 2, 7, 9)])
def test_head_16bit_maps_match_the_fp32_kernel_on_the_same_values(dtype, shape):
    """16-bit maps are consumed natively: statistics identical to the fp32 kernel on the up-cast values, gradient = the
    fp32 gradient rounded to nearest even into the map's type (fast 64x64 / 128x128 paths, float4-able and scalar shapes)."""
    from lc_amd.ptnet import spatial_softargmax_2d_std, softargmax_2d_std

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(sum(shape))
    lg16 = (torch.randn(shape, generator=g) * 3).to(dtype).to(dev).requires_grad_(True)
    lg32 = lg16.detach().float().requires_grad_(True)
    ct_m, ct_s = torch.randn(shape[:2] + (2,), generator=g).to(dev), torch.randn(shape[:2] + (2,), generator=g).to(dev)
    m16, s16 = spatial_softargmax_2d_std(lg16)
    m32, s32 = spatial_softargmax_2d_std(lg32)
    assert m16.dtype == torch.float32 and torch.equal(m16, m32) and torch.equal(s16, s32)
    (g16,) = torch.autograd.grad((m16 * ct_m).sum() + (s16 * ct_s).sum(), lg16)
    (g32,) = torch.autograd.grad((m32 * ct_m).sum() + (s32 * ct_s).sum(), lg32)
    assert g16.dtype == dtype and torch.equal(g16, g32.to(dtype))
    # probability input (ptnet.softargmax_2d_std itself)
    p16 = lg16.detach().float().flatten(-2).softmax(-1).reshape(shape).to(dtype).requires_grad_(True)
    p32 = p16.detach().float().requires_grad_(True)
    a16, b16 = softargmax_2d_std(p16)
    a32, b32 = softargmax_2d_std(p32)
    assert torch.equal(a16, a32) and torch.equal(b16, b32)
    (h16,) = torch.autograd.grad((a16 * ct_m).sum() + (b16 * ct_s).sum(), p16)
    (h32,) = torch.autograd.grad((a32 * ct_m).sum() + (b32 * ct_s).sum(), p32)
    assert torch.equal(h16, h32.to(dtype))


def test_softargmax_1d_cov_matches_the_reference_formula():
    """ptnet.py:85-97 restated in fp64: mean = sum i p_i, cov = sum (i - mean)^2 p_i; forward and gradient."""
    from lc_amd.ptnet import softargmax_1d_cov

    g = torch.Generator().manual_seed(3)
    p = torch.rand(5, 7, 37, generator=g).softmax(-1)
    x = p.to("cuda:0").requires_grad_(True)
    m, c = softargmax_1d_cov(x)
    ct = torch.randn(5, 7, 2, generator=g)
    (gx,) = torch.autograd.grad((m * ct[..., 0].to(x.device)).sum() + (c * ct[..., 1].to(x.device)).sum(), x)
    p64 = p.double().requires_grad_(True)
    idx = torch.arange(37, dtype=torch.float64)
    m64 = (p64 * idx).sum(-1)
    c64 = (p64 * (idx - m64[..., None]) ** 2).sum(-1)
    (g64,) = torch.autograd.grad((m64 * ct[..., 0].double()).sum() + (c64 * ct[..., 1].double()).sum(), p64)
    assert m.shape == (5, 7) and (m.cpu().double() - m64).abs().max() <= 1e-5 and (c.cpu().double() - c64).abs().max() <= 1e-4
    assert (gx.cpu().double() - g64).abs().max() <= 1e-3 * g64.abs().max()


@pytest.mark.parametrize("path", golden_files("headc_"), ids=[case_name(p, "headc_") for p in golden_files("headc_")])
def test_head_vs_golden_survey_sizes(path):
    """(4,16,64,64) and (2,64,64,64) -- the sizes SURVEY.md 8c names, S = 64 being the metric's map count -- against outputs of
    the reference's ptnet.softargmax_2d_std: every map's mean/std, every map's input gradient through two random functionals,
    six maps' gradients in full (tests/golden/gen_golden.py: gen_head_compact)."""
    from lc_amd.ptnet import spatial_softargmax_2d_std
    from tests.test_oracle_head import check_compact, compact_case

    z, logits, ct_mean, ct_std, probe = compact_case(path)
    dev = torch.device("cuda:0")
    lg = logits.to(dev).requires_grad_(True)
    mean, std = spatial_softargmax_2d_std(lg)
    (g,) = torch.autograd.grad([mean, std], [lg], [ct_mean.to(dev), ct_std.to(dev)])
    check_compact(z, mean.detach(), std.detach(), g, probe, 2e-4, 2e-6, tol_map=2e-4)  # same bounds as test_head_vs_golden (fp32 kernel, __expf)
    # the fp32 reference run sits as close to the fp64 one as the kernel does
    assert (torch.from_numpy(z["f32_mean"]).double() - torch.from_numpy(z["f64_mean"])).abs().max().item() <= 2e-4


def _map_at(vals, dtype, off):
    """vals (fp32, CPU) in `dtype` in a fresh device buffer at storage offset `off` elements, as a contiguous view (ptnet keeps it in place)."""
    buf = torch.zeros(vals.numel() + off, dtype=dtype, device="cuda:0")
    x = buf[off:].view(vals.shape)
    x.copy_(vals.to(dtype).to("cuda:0"))
    return x


def _head_fwd_bwd(x, prob, ct_m, ct_s):
    from lc_amd.ptnet import spatial_softargmax_2d_std, softargmax_2d_std

    x = x.detach().requires_grad_(True)
    mean, std = (softargmax_2d_std if prob else spatial_softargmax_2d_std)(x)
    (g,) = torch.autograd.grad((mean * ct_m).sum() + (std * ct_s).sum(), x)
    return mean.detach(), std.detach(), g


# (H, W, storage offset) -> lc_head_fwd_kernel<T, NV, VEC>: VEC = 4 needs W % 4 == 0 and the map aligned to four elements (else 1),
# NV = the power of two >= ceil(H W / (256 VEC)); 64 x 64 and 128 x 128 maps with VEC = 4 take the dedicated kernels instead
HEAD_FORMS = {
    (1, 4): (24, 40, 0), (2, 4): (32, 48, 0), (4, 4): (48, 60, 0), (8, 4): (80, 96, 0),
    (16, 4): (100, 160, 0),  # 65 KB of LDS: above the 48 KB default, hipFuncSetAttribute raises the limit
    (32, 4): (176, 176, 0),  # 123 KB of LDS
    (1, 1): (7, 9, 0), (2, 1): (15, 25, 0), (4, 1): (30, 33, 0), (8, 1): (32, 48, 1), (16, 1): (50, 61, 0), (32, 1): (64, 100, 1),
}


@pytest.mark.parametrize("prob", [False, True], ids=["logits", "prob"])
@pytest.mark.parametrize("nv,vec", sorted(HEAD_FORMS), ids=[f"NV{n}_VEC{v}" for n, v in sorted(HEAD_FORMS)])
def test_head_fwd_forms_fp32_vs_fp64(nv, vec, prob, spread=False):
    """Every (NV, VEC) form of the generic single-pass forward on fp32 maps, logits and probabilities in, forward and backward against
    the float64 restatement (oracle/softargmax_oracle.py).  The backward forms these shapes reach: lc_head_bwd_kernel<float, 4, false>
    (W % 4 == 0; none of these widths divides 1024, so the column-fixed form is not taken) and <float, 1, false> (W % 4 != 0 or a misaligned
    map).  The gradient is also judged map by map (tests/rowwise.py); `spread` (the test below) scales each map's cotangents by 10^U(-2, 2)."""
    from oracle import softargmax_oracle as orc

    H, W, off = HEAD_FORMS[(nv, vec)]
    assert (4 if (W % 4 == 0 and off % 4 == 0) else 1) == vec and max(1, 1 << ((H * W + 256 * vec - 1) // (256 * vec) - 1).bit_length()) == nv
    g = torch.Generator().manual_seed(H * W + prob)
    lg = torch.randn(2, 3, H, W, generator=g) * 3
    vals = lg.flatten(-2).softmax(-1).reshape(lg.shape) if prob else lg
    ct_m, ct_s = torch.randn(2, 3, 2, generator=g), torch.randn(2, 3, 2, generator=g)
    if spread:
        scale = 10 ** (torch.rand(2, 3, 1, generator=g) * 4 - 2)
        ct_m, ct_s = ct_m * scale, ct_s * scale
    mean, std, gx = _head_fwd_bwd(_map_at(vals, torch.float32, off), prob, ct_m.to("cuda:0"), ct_s.to("cuda:0"))
    fn = orc.softargmax_2d_std if prob else orc.spatial_softargmax_2d_std
    v64 = vals.double().requires_grad_(True)
    m64, s64 = fn(v64)
    (g64,) = torch.autograd.grad((m64 * ct_m.double()).sum() + (s64 * ct_s.double()).sum(), v64)
    assert (mean.cpu().double() - m64.detach()).abs().max().item() <= 3e-4
    assert (std.cpu().double() - s64.detach()).abs().max().item() <= 3e-4
    assert rel_err(gx.cpu(), g64) <= 3e-4
    v32 = vals.clone().requires_grad_(True)
    m32, s32 = fn(v32)
    (g32,) = torch.autograd.grad((m32 * ct_m).sum() + (s32 * ct_s).sum(), v32)
    if spread:
        big = g64.abs().flatten(-2).amax(-1).flatten()
        assert big.max() / big.min() >= 100  # the maps' gradients differ in size by two decades and more
    rw.check_kept(f"head NV{nv} VEC{vec} {'prob' if prob else 'logits'} gradient per map", gx, g64, g32, 3e-4, rows=(-1, H, W))


@pytest.mark.parametrize("prob", [False, True], ids=["logits", "prob"])
@pytest.mark.parametrize("nv,vec", sorted(HEAD_FORMS), ids=[f"NV{n}_VEC{v}" for n, v in sorted(HEAD_FORMS)])
def test_head_fwd_forms_fp32_vs_fp64_with_cotangents_spread_over_four_decades(nv, vec, prob):
    """The same forms and maps with each map's cotangents scaled by 10^U(-2, 2): maps with small gradients sit in the same launch as maps
    with large ones, and each is judged against its own largest entry."""
    test_head_fwd_forms_fp32_vs_fp64(nv, vec, prob, spread=True)


@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16], ids=["f16", "bf16"])
@pytest.mark.parametrize("prob", [False, True], ids=["logits", "prob"])
@pytest.mark.parametrize("nv,vec", sorted(HEAD_FORMS), ids=[f"NV{n}_VEC{v}" for n, v in sorted(HEAD_FORMS)])
def test_head_fwd_forms_16bit_match_the_fp32_kernel(nv, vec, prob, dtype):
    """The same (NV, VEC) forms on fp16 / bf16 maps: statistics identical to the fp32 kernel's on the up-cast values at the same storage
    offset (the same form), gradient = that fp32 gradient rounded to the map's type.  16-bit backward forms: <T, 8, false> (W % 8 == 0, none
    of these widths divides 2048), <T, 4, false> (W % 8 == 4) and <T, 1, false>."""
    H, W, off = HEAD_FORMS[(nv, vec)]
    g = torch.Generator().manual_seed(H * W + 7 * prob)
    lg = torch.randn(2, 3, H, W, generator=g) * 3
    vals = (lg.flatten(-2).softmax(-1).reshape(lg.shape) if prob else lg).to(dtype).float()
    ct_m, ct_s = torch.randn(2, 3, 2, generator=g).to("cuda:0"), torch.randn(2, 3, 2, generator=g).to("cuda:0")
    m16, s16, g16 = _head_fwd_bwd(_map_at(vals, dtype, off), prob, ct_m, ct_s)
    m32, s32, g32 = _head_fwd_bwd(_map_at(vals, torch.float32, off), prob, ct_m, ct_s)
    assert torch.equal(m16, m32) and torch.equal(s16, s32)
    assert g16.dtype == dtype and torch.equal(g16, g32.to(dtype))


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("prob", [False, True], ids=["logits", "prob"])
@pytest.mark.parametrize("off", [4, 1], ids=["off4", "off1"])
def test_head_64x64_forms_at_offset_views(off, prob, dtype):
    """64 x 64 maps at a storage offset leave the aligned paths: 16-bit maps at offset 4 (8 bytes) take lc_head_fwd_rows_kernel<T, 16, 4>
    (float4-able but not 16-byte aligned) and lc_head_bwd_kernel<T, 4, .> instead of <T, 8, .>; offset 1 takes the generic forward
    <T, 16, 1> and the backward <T, 1, false>; fp32 maps at offset 4 (16 bytes) stay on the one-wave-per-map forward and <float, 4, .>.
    Against the fp64 restatement on the (exactly up-cast) map values; a 16-bit gradient may differ from it by its rounding to the type."""
    from oracle import softargmax_oracle as orc

    g = torch.Generator().manual_seed(off + 10 * prob)
    lg = torch.randn(3, 2, 64, 64, generator=g) * 3
    vals = (lg.flatten(-2).softmax(-1).reshape(lg.shape) if prob else lg).to(dtype).float()
    ct_m, ct_s = torch.randn(3, 2, 2, generator=g), torch.randn(3, 2, 2, generator=g)
    m, s, gx = _head_fwd_bwd(_map_at(vals, dtype, off), prob, ct_m.to("cuda:0"), ct_s.to("cuda:0"))
    v64 = vals.double().requires_grad_(True)
    m64, s64 = (orc.softargmax_2d_std if prob else orc.spatial_softargmax_2d_std)(v64)
    (g64,) = torch.autograd.grad((m64 * ct_m.double()).sum() + (s64 * ct_s.double()).sum(), v64)
    assert (m.cpu().double() - m64.detach()).abs().max().item() <= 3e-4
    assert (s.cpu().double() - s64.detach()).abs().max().item() <= 3e-4
    assert gx.dtype == dtype
    rnd = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[dtype]  # half an ulp, relative
    assert ((gx.cpu().double() - g64).abs() <= 3e-4 * g64.abs().max() + rnd * g64.abs()).all()


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_head_map_beyond_the_single_pass_limit_is_an_error(dtype):
    """200 x 200: H (W + 1) + W + H + 8 floats of LDS = 159 KB fit, but 40000 elements need NV = 64 > 32 (VEC = 4); 180 x 230 needs
    164 KB > 160 KB.  launch_head_fwd_t returns 3, the wrapper raises -- never a partial result."""
    from lc_amd.ptnet import spatial_softargmax_2d_std

    for H, W in ((200, 200), (180, 230)):
        x = torch.zeros(1, 1, H, W, dtype=dtype, device="cuda:0")
        with pytest.raises(RuntimeError, match=r"code 3\): map too large for the single-pass"):
            spatial_softargmax_2d_std(x)


@pytest.mark.parametrize("prob", [False, True], ids=["logits", "prob"])
def test_head_rows_kernel_with_misaligned_outputs(prob):
    """fp32 64 x 64 maps reach lc_head_fwd_rows_kernel<float, 16, 4> only when an output is not aligned for the one-wave-per-map kernel's
    wide stores (mean / std to 8 bytes, stats to 16): the C ABI called with outputs at an offset of one float, against the fp64 restatement
    and against the wrapper's (aligned) run of the same maps."""
    from lc_amd import _lib
    from lc_amd.ptnet import softargmax_2d_std, spatial_softargmax_2d_std
    from oracle import softargmax_oracle as orc

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(64 + prob)
    lg = torch.randn(3, 2, 64, 64, generator=g) * 3
    vals = lg.flatten(-2).softmax(-1).reshape(lg.shape) if prob else lg
    x = vals.to(dev)
    M = 6
    buf = torch.zeros(1 + 2 * M + 1 + 2 * M + 1 + 4 * M, device=dev)
    mean, std, stats = buf[1:1 + 2 * M], buf[2 + 2 * M:2 + 4 * M], buf[3 + 4 * M:3 + 8 * M]
    rc = _lib.load().lc_softargmax2d_fwd(_lib.ptr(x), 0, M, 64, 64, int(prob), _lib.ptr(mean), _lib.ptr(std), _lib.ptr(stats), _lib.stream_ptr(dev))
    _lib.check(rc, "lc_softargmax2d_fwd")
    m64, s64 = (orc.softargmax_2d_std if prob else orc.spatial_softargmax_2d_std)(vals.double())
    assert (mean.view(3, 2, 2).cpu().double() - m64).abs().max().item() <= 3e-4
    assert (std.view(3, 2, 2).cpu().double() - s64).abs().max().item() <= 3e-4
    ma, sa = (softargmax_2d_std if prob else spatial_softargmax_2d_std)(x)
    assert (mean.view(3, 2, 2) - ma).abs().max().item() <= 1e-4 and (std.view(3, 2, 2) - sa).abs().max().item() <= 1e-4
