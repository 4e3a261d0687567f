"""The same output element gets the same bits whether its tile leaves through a staged store (interior tile) or through the general path
(edge tile): the convolution, fused and lean-fused output stages of csrc/conv.hip, through ops_nn's single-op wrappers.  (The linear-layer
extras have this check in tests/test_gpu_vit_plan_shapes.py.)

Launch A is 300 pixels x cout channels, launch B its first 100 pixels and the last cout - cout % 64 channels alone: against a 128- or 64-channel
tile the window is interior in A (pixels 0-99 lie in A's first, full pixel tile) and, with 100 pixels, an edge tile in B.  x, w and the
residual are small integers, so every accumulator is exact and the same in both launches; scale, shift, bias and res_scale are non-dyadic
fp32, so what is compared is the output stage's own sequence of roundings.

Not covered on purpose: out_shift together with bias.  The staged fused store folds the bias into the shift before the affine, the general
path adds it after (the one recorded disagreement, csrc/conv.hip: epi_store_staged), so there the bits may differ by design."""
import pytest
import torch

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
P, PB, CIN = 300, 100, 32


@pytest.fixture(scope="module")
def nn():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from daliid_amd import ops_nn
    return ops_nn


def ints(g, *shape, lo=-3, hi=4):
    return torch.randint(lo, hi, shape, generator=g).to(bf16).cuda()


def vec(g, n, lo, hi):
    """non-dyadic fp32 values in [lo, hi), either sign"""
    v = lo + (hi - lo) * torch.rand(n, generator=g)
    return (v * torch.where(torch.rand(n, generator=g) < 0.3, -1.0, 1.0)).cuda()


def pack_bits(b):
    """[rows, C] bool -> mask bytes: bit e & 7 of byte e >> 3, e = row * C + c"""
    b = b.flatten().to(torch.int32).view(-1, 8)
    return (b << torch.arange(8, dtype=torch.int32, device=b.device)).sum(1).to(torch.uint8)


def unpack_bits(m, rows, C):
    return ((m.to(torch.int32).unsqueeze(1) >> torch.arange(8, dtype=torch.int32, device=m.device)) & 1).bool().view(rows, C)


def window(cout):
    return cout % 64, cout          # 136 -> [8, 136), 72 -> [8, 72), 64 -> [0, 64)


def same_bits(a, b):
    assert torch.equal(a.contiguous().view(torch.int16), b.contiguous().view(torch.int16)), \
        "%d of %d elements differ" % (int((a.view(torch.int16) != b.view(torch.int16)).sum()), a.numel())


def test_conv_forward(nn):
    g = torch.Generator().manual_seed(1)
    cout = 136
    lo, hi = window(cout)
    x, w = ints(g, 1, P, 1, CIN), ints(g, cout, 1, 1, CIN)
    ya = nn.conv2d_fwd(x, w).view(P, cout)
    yb = nn.conv2d_fwd(x[:, :PB].contiguous(), w[lo:hi].contiguous()).view(PB, hi - lo)
    same_bits(ya[:PB, lo:hi], yb)


def test_conv_dgrad_masked_residual(nn):
    g = torch.Generator().manual_seed(2)
    cm = 136                                                    # the GEMM's output channels: the data gradient's input channels
    lo, hi = window(cm)
    dy, wt = ints(g, 1, P, 1, CIN), ints(g, cm, 1, 1, CIN)
    res = ints(g, 1, P, 1, cm, lo=-40, hi=41)
    keep = (torch.rand(P, cm, generator=g) < 0.6).cuda()
    da = nn.conv2d_dgrad(dy, wt, (P, 1), residual=res, residual_mask=pack_bits(keep)).view(P, cm)
    db = nn.conv2d_dgrad(dy[:, :PB].contiguous(), wt[lo:hi].contiguous(), (PB, 1), residual=res[:, :PB, :, lo:hi].contiguous(),
                         residual_mask=pack_bits(keep[:PB, lo:hi])).view(PB, hi - lo)
    same_bits(da[:PB, lo:hi], db)


@pytest.mark.parametrize("additive", ["out_shift", "bias"])
def test_fused_stage(nn, additive):
    g = torch.Generator().manual_seed(3)
    cout = 136
    lo, hi = window(cout)
    x, w = ints(g, P, CIN), ints(g, cout, CIN)
    res = ints(g, P, cout, lo=-40, hi=41)
    scale, add, res_scale = vec(g, cout, 0.3, 1.7), vec(g, cout, 0.1, 9.0), vec(g, cout, 0.3, 1.7)
    gate = (torch.rand(P, cout, generator=g) < 0.7).cuda()

    def run(rows, c0, c1):
        return nn.conv1x1_fused(x[:rows], w[c0:c1].contiguous(), out_scale=scale[c0:c1].contiguous(), residual=res[:rows, c0:c1].contiguous(),
                                res_scale=res_scale[c0:c1].contiguous(), relu=True, want_bits=True, out_mask=pack_bits(gate[:rows, c0:c1]),
                                **{additive: add[c0:c1].contiguous()})
    (ya, ba), (yb, bb) = run(P, 0, cout), run(PB, lo, hi)
    same_bits(ya[:PB, lo:hi], yb)
    assert torch.equal(unpack_bits(ba, P, cout)[:PB, lo:hi], unpack_bits(bb, PB, hi - lo))
    assert bool((yb != 0).any()) and bool((yb == 0).any())      # the gate and the ReLU both bite


@pytest.mark.parametrize("cout", [64, 72])
def test_lean_fused_stage(nn, cout):
    """conv + BatchNorm affine + ReLU in one launch (conv2d_bn_act), against the 64 x 256 tile"""
    g = torch.Generator().manual_seed(4 + cout)
    lo, hi = window(cout)
    x, w = ints(g, 1, P, 1, CIN), ints(g, cout, 1, 1, CIN)
    scale, shift = vec(g, cout, 0.3, 1.7), vec(g, cout, 0.1, 9.0)
    ya = nn.conv2d_bn_act(x, w, scale, shift, relu=True).view(P, cout)
    yb = nn.conv2d_bn_act(x[:, :PB].contiguous(), w[lo:hi].contiguous(), scale[lo:hi].contiguous(), shift[lo:hi].contiguous(), relu=True).view(PB, hi - lo)
    same_bits(ya[:PB, lo:hi], yb)
