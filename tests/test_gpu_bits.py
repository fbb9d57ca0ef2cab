"""GPU parity of the binary-code decode kernels against goldens from the reference's floatbits.py."""
import numpy as np
import pytest
import torch

from tests import rowwise as rw
from tests.util import golden_files, case_name, rel_err

pytestmark = pytest.mark.gpu
FILES = golden_files("bits_")


@pytest.mark.parametrize("path", FILES, ids=[case_name(p, "bits_") for p in FILES])
def test_bits_decode_vs_reference(path):
    from lc_amd import floatbits as fb

    z = np.load(path)
    dev = torch.device("cuda:0")
    bits = [int(b) for b in z["bits"]]
    lg = torch.from_numpy(z["in_logits"]).to(dev).requires_grad_(True)
    raw = torch.from_numpy(z["in_raw_bits"]).to(dev)
    msk = torch.from_numpy(z["in_msk"]).to(dev)
    out = fb.nn_logits2noc_with_gt(lg, raw, bits, msk)
    (gl,) = torch.autograd.grad(out, lg, torch.from_numpy(z["in_ct"]).to(dev))
    assert rel_err(out.detach().cpu(), z["f64_noc_gt"]) <= 2e-6
    assert rel_err(gl.cpu(), z["f64_g_logits"]) <= 5e-6
    # per sample and coordinate (tests/rowwise.py): the channels of one coordinate's bits are a row; the same 5e-6 against the row's own largest
    # entry, the reference's fp32 run setting the bound where it exceeds that on a row
    for c, (lo, n) in enumerate(zip(np.cumsum([0] + bits[:-1]), bits)):
        cut = lambda t: torch.as_tensor(t)[:, lo:lo + n]  # noqa: E731
        rw.check_kept(f"bits g_logits coordinate {c}", cut(gl.cpu()), cut(z["f64_g_logits"]), cut(z["f32_g_logits"]), 5e-6)
    inf = fb.nn_logits2noc(lg.detach(), bits)
    assert rel_err(inf.cpu(), z["f64_noc_inf"]) <= 2e-6


def test_bits_strided_subset_and_zlmo_shape():
    """Sub-sample first, decode second (losses.py:163-184) on a 128x128 map with the zlmo bit budget."""
    from lc_amd import floatbits as fb
    from oracle import floatbits_oracle as orc

    g = torch.Generator().manual_seed(2)
    B, H, W, bits = 2, 128, 128, [7, 7, 6]
    noc = torch.rand(B, H, W, 3, generator=g) * 2 - 1
    mod, raw = fb.nn_noc2target(noc, bits)
    lg = (mod.float() * 2 - 1) * (torch.rand(B, sum(bits), H, W, generator=g) * 3 + 0.1)
    lg = torch.where(torch.rand(lg.shape, generator=g) < 0.1, -lg, lg)
    msk = torch.rand(B, H, W, generator=g) > 0.2
    dev = torch.device("cuda:0")
    x = lg.to(dev).requires_grad_(True)
    out = fb.decode_with_gt_strided(x, raw.to(dev), bits, msk.to(dev), sample=3, top_left=(1, 2))
    x64 = lg.double().requires_grad_(True)
    ref = orc.nn_logits2noc_with_gt(x64[..., 1::3, 2::3], raw[..., 1::3, 2::3], bits, msk[..., 1::3, 2::3]).flatten(1, 2)
    assert out.shape == ref.shape and rel_err(out.detach().cpu(), ref.detach()) <= 2e-6
    ct = torch.randn(out.shape, generator=g)
    (gk,) = torch.autograd.grad(out, x, ct.to(dev))
    (go,) = torch.autograd.grad(ref, x64, ct.double())
    assert rel_err(gk.cpu(), go) <= 5e-6


@pytest.mark.parametrize("H,W,sample,tl", [(6, 10, 1, (0, 0)), (5, 7, 2, (1, 0)), (8, 12, 1, (0, 0)), (8, 12, 2, (0, 1))])
def test_bits_odd_widths_take_the_scalar_path(H, W, sample, tl):
    """Row lengths that are not a multiple of four (one pixel per thread) and the float4 path agree with the oracle."""
    from lc_amd import floatbits as fb
    from oracle import floatbits_oracle as orc

    g = torch.Generator().manual_seed(H * 100 + W)
    B, bits = 3, [5, 4, 3]
    noc = torch.rand(B, H, W, 3, generator=g) * 2 - 1
    mod, raw = fb.nn_noc2target(noc, bits)
    lg = (mod.float() * 2 - 1) * (torch.rand(B, sum(bits), H, W, generator=g) * 3 + 0.1)
    lg = torch.where(torch.rand(lg.shape, generator=g) < 0.15, -lg, lg)
    msk = torch.rand(B, H, W, generator=g) > 0.3
    dev = torch.device("cuda:0")
    x = lg.to(dev).requires_grad_(True)
    out = fb.decode_with_gt_strided(x, raw.to(dev), bits, msk.to(dev), sample=sample, top_left=tl)
    x64 = lg.double().requires_grad_(True)
    sl = (Ellipsis, slice(tl[0], None, sample), slice(tl[1], None, sample))
    ref = orc.nn_logits2noc_with_gt(x64[sl], raw[sl], bits, msk[sl]).flatten(1, 2)
    assert out.shape == ref.shape and rel_err(out.detach().cpu(), ref.detach()) <= 2e-6
    ct = torch.randn(out.shape, generator=g)
    (gk,) = torch.autograd.grad(out, x, ct.to(dev))
    (go,) = torch.autograd.grad(ref, x64, ct.double())
    assert rel_err(gk.cpu(), go) <= 5e-6
    inf = fb.nn_logits2noc(lg.to(dev), bits)
    assert rel_err(inf.cpu(), orc.nn_logits2noc(lg.double(), bits)) <= 2e-6


@pytest.mark.parametrize("H,W,sample,tl,with_T", [(64, 64, 2, (1, 0), True), (32, 32, 1, (0, 0), True), (21, 30, 2, (0, 1), False), (16, 16, 1, (0, 0), False)])
def test_decode_with_the_coordinate_map_folded_in(H, W, sample, tl, with_T):
    """lc_bits_decode_gt_{fwd,bwd}2_f32: `noc * noc_scale` and the model transform `(xyz - T[:, :3, 3]) @ T[:, :3, :3]` of
    nn_out_to_xyz (losses.py:17-47) applied by the decode launches, against the plain decode followed by the torch ops (float64 on the
    oracle's decode): values and logit gradients."""
    from lc_amd import floatbits as fb
    from oracle import floatbits_oracle as orc

    g = torch.Generator().manual_seed(H + W)
    B, bits = 3, [6, 6, 5]
    noc = torch.rand(B, H, W, 3, generator=g) * 2 - 1
    mod, raw = fb.nn_noc2target(noc, bits)
    lg = (mod.float() * 2 - 1) * (torch.rand(B, sum(bits), H, W, generator=g) * 3 + 0.1)
    lg = torch.where(torch.rand(lg.shape, generator=g) < 0.1, -lg, lg)
    msk = torch.rand(B, H, W, generator=g) > 0.2
    scale = torch.rand(B, 3, generator=g) * 100 + 20
    T = None
    if with_T:
        q, _ = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))
        T = torch.eye(4).repeat(B, 1, 1)
        T[:, :3, :3] = q
        T[:, :3, 3] = torch.randn(B, 3, generator=g) * 5
    dev = torch.device("cuda:0")
    x = lg.to(dev).requires_grad_(True)
    out = fb.decode_with_gt_strided(x, raw.to(dev), bits, msk.to(dev), sample=sample, top_left=tl, out_scale=scale.to(dev),
                                    out_xform=None if T is None else T.to(dev))
    x64 = lg.double().requires_grad_(True)
    sl = (Ellipsis, slice(tl[0], None, sample), slice(tl[1], None, sample))
    ref = orc.nn_logits2noc_with_gt(x64[sl], raw[sl], bits, msk[sl]).flatten(1, 2) * scale.double()[:, None]
    if T is not None:
        ref = (ref - T.double()[:, None, :3, 3]) @ T.double()[:, :3, :3]
    assert out.shape == ref.shape and rel_err(out.detach().cpu(), ref.detach()) <= 2e-6
    ct = torch.randn(out.shape, generator=g)
    (gk,) = torch.autograd.grad(out, x, ct.to(dev))
    (go,) = torch.autograd.grad(ref, x64, ct.double())
    assert rel_err(gk.cpu(), go) <= 5e-6


@pytest.mark.parametrize("H,W,with_T", [(64, 64, True), (30, 21, True), (128, 128, False)])
def test_inference_decode_straight_to_xyz_planes(H, W, with_T):
    """lc_bits_decode3 (Gray decode + noc_scale + model transform, written as (B,3,H,W) planes) against
    `nn_out_to_xyz(..., inference=True).permute(0, 3, 1, 2)`: the decode itself bit for bit (same kernel body), the coordinate map to
    fp32 rounding of a 3-term product sum."""
    from lc_amd import floatbits as fb
    from lc_amd.losses import nn_out_to_xyz

    g = torch.Generator().manual_seed(H * W)
    B, bits = 3, [7, 6, 6]
    dev = torch.device("cuda:0")
    lg = (torch.randn(B, sum(bits), H, W, generator=g) * 2).to(dev)
    scale = (torch.rand(B, 3, generator=g) * 100 + 20).to(dev)
    T = None
    if with_T:
        q, _ = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))
        T = torch.eye(4).repeat(B, 1, 1)
        T[:, :3, :3] = q
        T[:, :3, 3] = torch.randn(B, 3, generator=g) * 5
        T = T.to(dev)
    got = fb.nn_logits2xyz_planes(lg, bits, scale, T)
    want = nn_out_to_xyz(lg, scale, model_transform=T, bit_cnt=bits, inference=True).permute(0, 3, 1, 2)
    assert got.shape == want.shape == (B, 3, H, W) and got.is_contiguous()
    if T is None:
        assert torch.equal(got, want.contiguous())
    else:
        assert (got - want).abs().max() <= 2e-5 * want.abs().max()


@pytest.mark.parametrize("H,W,sample,tl,bits,masked", [
    (128, 128, 3, (1, 2), [7, 7, 7], True),    # zlmo's training shape: tiles of 4 rows (42 sampled columns x 2 rows x 3 axes = 252 items)
    (128, 128, 3, (0, 0), [7, 7, 7], True),    # 43 sampled columns: tiles of 3 rows
    (128, 128, 3, (2, 1), [7, 7, 6], False),   # no object mask
    (64, 64, 2, (1, 1), [7, 7, 6], True),      # glmo-sized maps with binary heads, stride 2: tiles of 4 rows, two sampled rows each
    (30, 64, 2, (0, 1), [5, 4, 3], True),      # a height the tile rows do not divide
    (31, 32, 3, (2, 0), [6, 6, 6], True),
    (16, 128, 2, (1, 0), [9, 10, 3], True),    # axes of more than eight bits: a second round of requests
    (20, 24, 2, (0, 0), [5, 5, 5], True),      # 24 / 8 = 3 pieces per row does not divide the workgroup: the flat backward kernel
    (24, 40, 4, (3, 1), [5, 5, 5], True),      # stride 4: the flat backward kernel, the wide forward kernel
])
def test_strided_training_decode_launch_forms(H, W, sample, tl, bits, masked):
    """The strided-subset forms of round 6 (`lc_bits_decode_gt_fwd_wide_kernel`: every request of a pixel in flight at once;
    `lc_bits_decode_gt_bwd_tile_kernel<E, T, SAMPLE, R>`: zero rows first, one (pixel, axis) item per thread, every 16-byte piece written once) and
    the shapes that fall back to the flat kernels, against the float64 oracle (floatbits.py:130-160 restated) with the callers' coordinate map
    folded in; then fp16 / bf16 logits: the result of the fp32 kernels on the up-cast values, bit for bit (gradient: rounded once to the map's type)."""
    from lc_amd import floatbits as fb
    from oracle import floatbits_oracle as orc

    g = torch.Generator().manual_seed(H * 1000 + W * 10 + sample)
    B = 3
    noc = torch.rand(B, H, W, 3, generator=g) * 2 - 1
    mod, raw = fb.nn_noc2target(noc, bits)
    lg = (mod.float() * 2 - 1) * (torch.rand(B, sum(bits), H, W, generator=g) * 3 + 0.1)
    lg = torch.where(torch.rand(lg.shape, generator=g) < 0.15, -lg, lg)
    msk = (torch.rand(B, H, W, generator=g) > 0.3) if masked else None
    scale = torch.rand(B, 3, generator=g) * 60 + 20
    ang = torch.rand(B, generator=g) * 0.6 - 0.3
    T = torch.eye(4).repeat(B, 1, 1)
    T[:, 0, 0] = T[:, 1, 1] = ang.cos()
    T[:, 0, 1], T[:, 1, 0] = -ang.sin(), ang.sin()
    T[:, :3, 3] = torch.randn(B, 3, generator=g) * 2
    dev = torch.device("cuda:0")
    dm = None if msk is None else msk.to(dev)
    x = lg.to(dev).requires_grad_(True)
    out = fb.decode_with_gt_strided(x, raw.to(dev), bits, dm, sample=sample, top_left=tl, out_scale=scale.to(dev), out_xform=T.to(dev))
    x64 = lg.double().requires_grad_(True)
    sl = (Ellipsis, slice(tl[0], None, sample), slice(tl[1], None, sample))
    m64 = torch.ones(B, H, W, dtype=torch.bool) if msk is None else msk
    noc64 = orc.nn_logits2noc_with_gt(x64[sl], raw[sl], bits, m64[sl]).flatten(1, 2)
    ref = (noc64 * scale.double()[:, None] - T.double()[:, None, :3, 3]) @ T.double()[:, :3, :3]
    assert out.shape == ref.shape and rel_err(out.detach().cpu(), ref.detach()) <= 2e-6
    ct = torch.randn(out.shape, generator=g)
    (gk,) = torch.autograd.grad(out, x, ct.to(dev))
    (go,) = torch.autograd.grad(ref, x64, ct.double())
    assert rel_err(gk.cpu(), go) <= 5e-6
    off = torch.ones(H, W, dtype=torch.bool)
    off[tl[0]::sample, tl[1]::sample] = False
    assert float(gk[..., off.to(dev)].abs().max()) == 0.0  # nothing off the sampled pixels
    for dt in (torch.float16, torch.bfloat16):
        xh = lg.to(dev).to(dt).requires_grad_(True)
        xf = xh.detach().float().requires_grad_(True)
        oh = fb.decode_with_gt_strided(xh, raw.to(dev), bits, dm, sample=sample, top_left=tl, out_scale=scale.to(dev), out_xform=T.to(dev))
        of = fb.decode_with_gt_strided(xf, raw.to(dev), bits, dm, sample=sample, top_left=tl, out_scale=scale.to(dev), out_xform=T.to(dev))
        assert torch.equal(oh, of)
        (gh,), (gf,) = torch.autograd.grad(oh, xh, ct.to(dev)), torch.autograd.grad(of, xf, ct.to(dev))
        assert gh.dtype == dt and torch.equal(gh, gf.to(dt))


def _code_case(g, B, H, W, bits):
    from lc_amd import floatbits as fb

    noc = torch.rand(B, H, W, 3, generator=g) * 2 - 1
    mod, raw = fb.nn_noc2target(noc, bits)
    lg = (mod.float() * 2 - 1) * (torch.rand(B, sum(bits), H, W, generator=g) * 3 + 0.1)
    lg = torch.where(torch.rand(lg.shape, generator=g) < 0.15, -lg, lg)
    msk = torch.rand(B, H, W, generator=g) > 0.3
    return lg, raw, msk


# (sample, rows per tile) -> fp32 (W, left), 16-bit (W, left).  launch_bits_decode_gt_bwd: E = 16 bytes / element, per_row = W / E pieces
# of a row (dividing 256), Wn = ceil((W - left) / sample); rows per tile = the largest R <= 4 with ceil(R / sample) Wn 3 <= 256 and
# R per_row <= 256.  (2, 3) has no shape: R = 3 and 4 give the same ceil(R / 2), and no per_row dividing 256 lies in (64, 256 / 3].
TILE_FORMS = {
    (2, 1): ((1024, 900), (2048, 1900)),  # per_row = 256: one row per tile; a left margin keeps Wn <= 85
    (2, 2): ((128, 0), (128, 0)),
    (2, 4): ((64, 0), (64, 0)),
    (3, 1): ((1024, 900), (2048, 1900)),
    (3, 2): ((512, 300), (1024, 800)),  # per_row = 128
    (3, 3): ((128, 0), (128, 0)),  # zlmo: 128 wide, every third pixel
    (3, 4): ((64, 0), (64, 0)),
}


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
@pytest.mark.parametrize("S,RR", sorted(TILE_FORMS), ids=[f"S{s}_RR{r}" for s, r in sorted(TILE_FORMS)])
def test_bits_tile_backward_forms(S, RR, dtype):
    """Each lc_bits_decode_gt_bwd_tile_kernel<E, T, S, RR> the launcher can pick: a strided subset (sample S, a row offset of 1 and the
    listed column offset) whose row width gives RR rows per tile, over seven rows (a partial last tile).  fp32 against the fp64 oracle;
    fp16 / bf16 maps against the fp32 kernel on the up-cast logits: the same decode, the gradient rounded to the map's type."""
    from lc_amd import floatbits as fb
    from oracle import floatbits_oracle as orc

    W, left = TILE_FORMS[(S, RR)][dtype != torch.float32]
    E = 4 if dtype == torch.float32 else 8
    Wn, per_row = (W - left + S - 1) // S, W // E
    assert 256 % per_row == 0 and max(R for R in range(1, 5) if (R + S - 1) // S * Wn * 3 <= 256 and R * per_row <= 256) == RR
    g = torch.Generator().manual_seed(W * 10 + S)
    B, H, bits = 2, 7, [5, 4, 3]
    lg, raw, msk = _code_case(g, B, H, W, bits)
    lg = lg.to(dtype).float()
    dev = torch.device("cuda:0")
    tl = (1, left)
    x = lg.to(dtype).to(dev).requires_grad_(True)
    out = fb.decode_with_gt_strided(x, raw.to(dev), bits, msk.to(dev), sample=S, top_left=tl)
    ct = torch.randn(out.shape, generator=g)
    (gk,) = torch.autograd.grad(out, x, ct.to(dev))
    assert gk.dtype == dtype
    if dtype != torch.float32:
        x32 = lg.to(dev).requires_grad_(True)
        out32 = fb.decode_with_gt_strided(x32, raw.to(dev), bits, msk.to(dev), sample=S, top_left=tl)
        (g32,) = torch.autograd.grad(out32, x32, ct.to(dev))
        assert torch.equal(out, out32) and torch.equal(gk, g32.to(dtype))
        return
    x64 = lg.double().requires_grad_(True)
    sl = (Ellipsis, slice(tl[0], None, S), slice(tl[1], None, S))
    ref = orc.nn_logits2noc_with_gt(x64[sl], raw[sl], bits, msk[sl]).flatten(1, 2)
    assert out.shape == ref.shape and rel_err(out.detach().cpu(), ref.detach()) <= 2e-6
    (go,) = torch.autograd.grad(ref, x64, ct.double())
    assert rel_err(gk.cpu(), go) <= 5e-6


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16, torch.bfloat16], ids=["f32", "f16", "bf16"])
def test_bits_more_than_65535_samples_take_the_generic_forward(dtype):
    """B = 65536 1 x 1 maps: the grid's y dimension cannot hold the batch, so the strided forward leaves the wide kernel
    (lc_bits_decode_gt_fwd_wide_kernel: B <= 65535) for lc_bits_decode_gt_fwd_kernel<1, T>, and the backward takes
    lc_bits_decode_gt_bwd_kernel<1, T>.  Against the fp64 oracle."""
    from lc_amd import floatbits as fb
    from oracle import floatbits_oracle as orc

    g = torch.Generator().manual_seed(65536)
    B, bits = 65536, [3, 2, 2]
    lg, raw, msk = _code_case(g, B, 1, 1, bits)
    lg = lg.to(dtype).float()
    dev = torch.device("cuda:0")
    x = lg.to(dtype).to(dev).requires_grad_(True)
    out = fb.nn_logits2noc_with_gt(x, raw.to(dev), bits, msk.to(dev))
    ct = torch.randn(out.shape, generator=g)
    (gk,) = torch.autograd.grad(out, x, ct.to(dev))
    x64 = lg.double().requires_grad_(True)
    ref = orc.nn_logits2noc_with_gt(x64, raw, bits, msk)
    assert rel_err(out.detach().cpu(), ref.detach()) <= 2e-6
    (go,) = torch.autograd.grad(ref, x64, ct.double())
    rnd = {torch.float32: 0.0, torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8}[dtype]  # half an ulp of the gradient's type, relative
    assert ((gk.cpu().double() - go).abs() <= 5e-6 * go.abs().max() + rnd * go.abs()).all()


def _oracle_floor(bound, f32, f64):
    """The file's bound, or twice the error of the oracle's own fp32 run against its fp64 run where that is larger."""
    return max(bound, 2.0 * rel_err(f32, f64))


# every axis length at which a walk of the channels changes: the smallest axis, the ends of the first, second and third round of eight, the C ABI's limit
ROUND_EDGE_BITS = [[1, 8, 9], [16, 17, 1], [24, 1, 8]]


def _bits_id(bits):
    return "-".join(str(b) for b in bits)


@pytest.mark.parametrize("H,W", [(3, 8), (3, 5)], ids=["3x8", "3x5"])  # four pixels per thread / one pixel per thread
@pytest.mark.parametrize("bits", ROUND_EDGE_BITS, ids=_bits_id)
def test_gray_decode_at_every_round_edge(bits, H, W):
    """The inference (Gray) decode on axes of 1, 8, 9, 16, 17 and 24 bits -- decode_gray's first round alone, its second and its third --
    through the three forms that share its pixel body: `nn_logits2noc` against the fp64 oracle, `nn_logits2xyz_planes` against
    `nn_out_to_xyz(..., inference=True)`, `decode_selected_rows` against the planes gathered at a permutation of every pixel (a sample
    with count 0 and everything behind a count left alone); fp16 / bf16 logits: the fp32 kernels on the up-cast values, bit for bit."""
    from lc_amd import floatbits as fb
    from lc_amd.losses import nn_out_to_xyz
    from oracle import floatbits_oracle as orc

    g = torch.Generator().manual_seed(sum(b * 31 ** i for i, b in enumerate(bits)) + W)
    B, C, N = 2, sum(bits), H * W
    dev = torch.device("cuda:0")
    lg = torch.randn(B, C, H, W, generator=g)
    scale = (torch.rand(B, 3, generator=g) * 100 + 20).to(dev)
    q, _ = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))
    T = torch.eye(4).repeat(B, 1, 1)
    T[:, :3, :3] = q
    T[:, :3, 3] = torch.randn(B, 3, generator=g) * 5
    T = T.to(dev)
    index = torch.stack([torch.randperm(N, generator=g) for _ in range(B)]).int().to(dev)
    counts = torch.tensor([0, N], dtype=torch.int32, device=dev)
    sentinel = -12345.0

    def rows(x, xf):
        out = torch.full((B, N, 3), sentinel, device=dev)
        return fb.decode_selected_rows(x, bits, index, counts, out, noc_scale=scale, model_transform=xf)

    def gathered(planes):  # (B,3,H,W) -> (B,N,3) in the order of `index`, the sentinel behind each sample's count
        pts = torch.gather(planes.flatten(2), 2, index.long()[:, None, :].expand(B, 3, N)).mT.contiguous()
        return torch.where((torch.arange(N, device=dev)[None, :] < counts[:, None])[..., None], pts, torch.full_like(pts, sentinel))

    x = lg.to(dev)
    ref64 = orc.nn_logits2noc(lg.double(), bits)
    bound = _oracle_floor(2e-6, orc.nn_logits2noc(lg, bits), ref64)  # 2e-6 in every case: the oracle's fp32 run is within 1.2e-7 of its fp64 run
    noc = fb.nn_logits2noc(x, bits)
    err = rel_err(noc.cpu(), ref64)
    print(f"gray decode {bits} {H}x{W}: rel_err {err:.3g}, bound {bound:.3g}")
    assert noc.shape == (B, H, W, 3) and err <= bound
    planes = fb.nn_logits2xyz_planes(x, bits, scale, None)
    assert torch.equal(planes, nn_out_to_xyz(x, scale, model_transform=None, bit_cnt=bits, inference=True).permute(0, 3, 1, 2).contiguous())
    planes_T = fb.nn_logits2xyz_planes(x, bits, scale, T)
    want_T = nn_out_to_xyz(x, scale, model_transform=T, bit_cnt=bits, inference=True).permute(0, 3, 1, 2)
    assert (planes_T - want_T).abs().max() <= 2e-5 * want_T.abs().max()
    assert torch.equal(rows(x, None), gathered(planes)) and torch.equal(rows(x, T), gathered(planes_T))
    for dt in (torch.float16, torch.bfloat16):
        xh = x.to(dt)
        xf = xh.float()
        assert torch.equal(fb.nn_logits2noc(xh, bits), fb.nn_logits2noc(xf, bits))
        for xform in (None, T):
            assert torch.equal(fb.nn_logits2xyz_planes(xh, bits, scale, xform), fb.nn_logits2xyz_planes(xf, bits, scale, xform))
            assert torch.equal(rows(xh, xform), rows(xf, xform))


@pytest.mark.parametrize("H,W,sample,tl", [
    (5, 16, 1, (0, 0)),  # forward and backward: the flat kernels, four pixels per thread
    (5, 5, 1, (0, 0)),   # the wide forward; the flat backward, one pixel per thread
    (5, 16, 2, (1, 0)),  # the wide forward; the tiled backward (16 / 4 = 4 pieces per row for fp32, 16 / 8 = 2 for the 16-bit types), a partial last tile
], ids=["5x16", "5x5", "5x16_s2"])
@pytest.mark.parametrize("bits", ROUND_EDGE_BITS[1:], ids=_bits_id)
def test_training_decode_at_every_round_edge(bits, H, W, sample, tl):
    """The training decode on axes of 1, 8, 16, 17 and 24 bits (9: `[9, 10, 3]` in test_strided_training_decode_launch_forms) -- one, two
    and three rounds of eight channels -- through every kernel that walks them, with an object mask: values and logit gradients of the fp32 kernels against the fp64 oracle, no gradient off the
    sampled pixels; fp16 / bf16 logits: the fp32 kernels on the up-cast values, bit for bit (gradient: rounded once to the map's type).
    One logit in twenty contradicts its ground-truth bit, so that the first wrong bit of an axis falls into each of its rounds."""
    from lc_amd import floatbits as fb
    from oracle import floatbits_oracle as orc

    g = torch.Generator().manual_seed(sum(b * 31 ** i for i, b in enumerate(bits)) + H * W + sample)
    B = 2
    noc = torch.rand(B, H, W, 3, generator=g) * 2 - 1
    mod, raw = fb.nn_noc2target(noc, bits)
    lg = (mod.float() * 2 - 1) * (torch.rand(B, sum(bits), H, W, generator=g) * 3 + 0.1)
    lg = torch.where(torch.rand(lg.shape, generator=g) < 0.05, -lg, lg)
    msk = torch.rand(B, H, W, generator=g) > 0.3
    dev = torch.device("cuda:0")
    sl = (Ellipsis, slice(tl[0], None, sample), slice(tl[1], None, sample))

    def oracle(dtype):
        xo = lg.to(dtype).requires_grad_(True)
        out = orc.nn_logits2noc_with_gt(xo[sl], raw[sl], bits, msk[sl]).flatten(1, 2)
        return xo, out

    x64, ref = oracle(torch.float64)
    x32, ref32 = oracle(torch.float32)
    ct = torch.randn(ref.shape, generator=g)
    (go,), (go32,) = torch.autograd.grad(ref, x64, ct.double()), torch.autograd.grad(ref32, x32, ct)
    # 2e-6 and 5e-6 in every case: the oracle's fp32 run is within 1.4e-7 (values) and 1.6e-7 (gradients) of its fp64 run
    bound_v, bound_g = _oracle_floor(2e-6, ref32.detach(), ref.detach()), _oracle_floor(5e-6, go32, go)
    x = lg.to(dev).requires_grad_(True)
    out = fb.decode_with_gt_strided(x, raw.to(dev), bits, msk.to(dev), sample=sample, top_left=tl)
    (gk,) = torch.autograd.grad(out, x, ct.to(dev))
    err_v, err_g = rel_err(out.detach().cpu(), ref.detach()), rel_err(gk.cpu(), go)
    print(f"training decode {bits} {H}x{W} sample {sample}: values {err_v:.3g} (bound {bound_v:.3g}), gradients {err_g:.3g} (bound {bound_g:.3g})")
    assert out.shape == ref.shape and err_v <= bound_v
    assert err_g <= bound_g
    off = torch.ones(H, W, dtype=torch.bool)
    off[tl[0]::sample, tl[1]::sample] = False
    if off.any():
        assert float(gk[..., off.to(dev)].abs().max()) == 0.0  # nothing off the sampled pixels
    for dt in (torch.float16, torch.bfloat16):
        xh = lg.to(dev).to(dt).requires_grad_(True)
        xf = xh.detach().float().requires_grad_(True)
        oh = fb.decode_with_gt_strided(xh, raw.to(dev), bits, msk.to(dev), sample=sample, top_left=tl)
        of = fb.decode_with_gt_strided(xf, raw.to(dev), bits, msk.to(dev), sample=sample, top_left=tl)
        assert torch.equal(oh, of)
        (gh,), (gf,) = torch.autograd.grad(oh, xh, ct.to(dev)), torch.autograd.grad(of, xf, ct.to(dev))
        assert gh.dtype == dt and torch.equal(gh, gf.to(dt))
        if off.any():
            assert float(gh[..., off.to(dev)].abs().max()) == 0.0
