"""GPU parity of the igemm_conv_ring_kernel instantiations that no other bit-exact test launches (tests/test_conv_dispatch_cpu.py lists what
every such test reaches, and asserts that with CASES nothing is left): the linear-layer output stage (Epi::LIN) on the 128 x 128 and the
128 x 256 k-tile-32 tiles, which the ViT plan's sizes pass by.  Small integers, which bf16 holds exactly and whose sums fp32 holds exactly, and
power-of-two row factors: every result must equal torch's CPU fp32 result rounded once to bf16, BIT FOR BIT.

Shapes: the smallest that reach the entry through the chooser's own thresholds, with a ragged last tile in both directions (interior tiles
take the staged linear-extras block, edge tiles the general path) and a k-tile count that wraps the 3-stage ring and is no multiple of it."""
import pytest
import torch

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
LIN = 64        # include/daliid_debug.h: DALI_DEBUG_CONV_LIN

# (entry, rows, K, N, flags of the launch for dali_debug_conv_kernel_name)
CASES = [
    ("DMA128_LIN", 300, 160, 136, LIN),        # conv_pick_cfg's default tile: 2 x 3 tiles (128 + 8 channels, 128 + 128 + 44 rows), 5 k-tiles
    ("WG128_LIN", 16500, 544, 264, LIN),       # K >= 512, >= 16384 rows, >= 256 outputs, K % 64 != 0: 3 x 65 tiles (.. + 8 channels, .. + 116 rows), 17 k-tiles
]


@pytest.fixture(scope="module")
def V():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from daliid_amd import ops_vit
    return ops_vit


def _ints(lo, hi, shape, gen, density=1.0):
    t = torch.randint(lo, hi + 1, shape, generator=gen).float()
    if density < 1.0:
        t = t * (torch.rand(shape, generator=gen) < density).float()
    return t


@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_linear_extras_exact_integers(V, case):
    _, rows, K, N, _ = case
    gen = torch.Generator().manual_seed(rows + 3 * K + N)
    x = _ints(-2, 2, (rows, K), gen)
    w = _ints(-2, 2, (N, K), gen, density=0.5)
    bias = _ints(-8, 8, (N,), gen)
    res = _ints(-16, 16, (rows, N), gen)
    rs = torch.tensor([0.0, 0.5, 1.0, 2.0, 0.25])[torch.randint(0, 5, (rows,), generator=gen)]
    pre = x @ w.t() + bias                             # |sums| <= 4 K + 8 < 2^24: exact in fp32 in any order
    xg, wg, bg = x.to(bf16).cuda(), w.to(bf16).cuda(), bias.cuda()
    # bias, DropPath row factor, residual: ((acc + bias) x rs) + res, every step exact, one rounding to bf16
    y = V.linear_fwd_scaled(xg, wg, rs.cuda(), bias=bg, residual=res.to(bf16).cuda())
    ref = (pre * rs[:, None] + res).to(bf16)
    assert torch.equal(y.cpu(), ref), (y.cpu().float() - ref.float()).abs().max()
    # the pre-activation copy (O2) beside the output
    y, pre_k = V.linear_fwd(xg, wg, bg, want_pre=True)
    assert torch.equal(y.cpu(), pre.to(bf16)) and torch.equal(pre_k.cpu(), pre.to(bf16))
