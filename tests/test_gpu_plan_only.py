"""Exact GPU checks of the code that only the net plan (csrc/resnet_plan.hip) reaches, against plain torch references of the same operations.

Every convolution, normalisation, pooling and loss kernel with a single-op C entry point is compared bit for bit elsewhere; the pieces below have
no such entry point and were covered only by whole-net comparisons at 4e-2 / 4e-3, inside which a deterministic indexing defect fits:

1. the stem weight gradient: stem_pack_image -> the split plan of (Cout, 224, P, taps 7) -> the weight-gradient GEMM on the packed image with the
   plan's gather geometry (stem_geom) -> stem_unpack_wgrad, through dali_debug_stem_wgrad; the packed image and the packed stem weight; and the
   plan's own conv1.weight gradient against the same entry on the plan's own d_raw0;
2. the bf16 weight images (cast, batched transposes with more than one 56-job chunk), the batched eval BatchNorm coefficients (two chunks) and the
   folded hi + lo weight image of the inference forward, read through dali_resnet_debug_tensor;
3. the head-pool backward with its ReLU gate (dali_debug_head_pool_bwd_masked);
4. the column sums that ride on the weight-gradient GEMMs (the [colsum] instantiations), through dali_bnlin_fwd / dali_bnlin_bwd on small integers.

Small integers make every product and every fp32 partial sum exact in any order of additions (each test asserts the bound it relies on), so
torch.equal applies.  The library is built with -ffp-contract=off: a one- or two-operation fp32 expression evaluated in the same order by torch
on the CPU is the bit-exact expectation of such a kernel.

WG_WG[1] (the plain 8-wave 128 x 256 weight-gradient kernel with column sums) takes the launches of cfg 2 with more than 100 output tiles of
128 x 256.  Both entry points can reach it.  dali_bnlin_fwd's Gram GEMM is w x w, and ceil(w / 128) * ceil(w / 256) > 100 first holds at w = 1824
(15 x 8 tiles); P = 16384 is the smallest pixel count of cfg 2.  dali_bnlin_bwd's GEMM is C x w with w <= 640 (its row kernel refuses more), so it
needs C >= 4352 at w = 640: a dz of 71 M elements against 30 M for the forward's operand.  The forward shape is the smallest; it is the last test
of this file (forward only: the backward refuses w = 1824)."""
import ctypes
import functools
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.resnet50_reid import ResNet50ReID as OracleNet

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
_T0 = time.time()


@pytest.fixture(scope="module")
def ops_nn():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from daliid_amd import ops_nn
    yield ops_nn
    print("\ntests/test_gpu_plan_only.py: %.1f s in all" % (time.time() - _T0))


def _lib_dbg():
    """the diagnostic entry points (include/daliid_debug.h), bound here: nothing under daliid_amd/ binds them"""
    from daliid_amd import _lib
    L = _lib.lib()
    vp, ci = ctypes.c_void_p, ctypes.c_int
    L.dali_debug_wgrad_splits.argtypes = [ci] * 5
    L.dali_debug_stem_wgrad.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, vp]
    L.dali_debug_head_pool_bwd_masked.argtypes = [vp, vp, vp, vp, ci, ci, ci, ci, vp, vp]
    return _lib, L


def bits16(t):
    """bit patterns of a bf16 tensor"""
    assert t.dtype == bf16
    return t.contiguous().view(torch.int16)


def bits32(t):
    assert t.dtype == torch.float32
    return t.contiguous().view(torch.int32)


def bits_of(keep):
    """mask bytes in the layout of bits_of in test_gpu_bnlin.py: bit t of byte i = keep.flatten()[8 i + t]"""
    b = keep.flatten().to(torch.uint8).reshape(-1, 8)
    return (b * (2 ** torch.arange(8, dtype=torch.uint8, device=keep.device))).sum(1).to(torch.uint8)


def ints(shape, gen, lo, hi, density=1.0):
    t = torch.randint(lo, hi + 1, shape, generator=gen).float()
    if density < 1.0:
        t = t * (torch.rand(shape, generator=gen) < density).float()
    return t


# ---- 1. stem weight gradient --------------------------------------------------------------------------------------------------------------
def stem_splits(L, Cout, P):
    """(splits, pixels per split, pixels of the last split) of the plan's stem weight gradient, from the library's own split plan"""
    sp = L.dali_debug_wgrad_splits(Cout, 224, P, 7, 0)
    pps = (-(-P // sp) + 31) // 32 * 32                  # wgrad_plan: the per-split share rounded up to whole k-steps of 32 pixels
    assert sp >= 1 and -(-P // pps) == sp, (sp, pps)
    return sp, pps, P - (sp - 1) * pps


# (N, H, W, Cout) -> what the split plan must show for the case to reach its path (checked against dali_debug_wgrad_splits, no hard-coded count)
STEM_CASES = [(2, 32, 32, 32), (3, 64, 32, 64), (2, 256, 128, 64), (43, 32, 48, 64), (8, 256, 128, 64)]


@functools.lru_cache(maxsize=None)
def stem_case(case):
    """images in [-3, 3], d_raw0 in [-2, 2] at density 0.5 (NHWC), and torch's CPU fp32 weight gradient in OHWI"""
    N, H, W, Cout = case
    P = N * (H // 2) * (W // 2)
    assert P * 3 * 2 < 2 ** 24                           # |image| <= 3, |d_raw0| <= 2: every partial sum is an integer below 2^24, exact in any order
    gen = torch.Generator().manual_seed(N * 1000 + H + W + Cout)
    x = ints((N, 3, H, W), gen, -3, 3)
    d = ints((N, Cout, H // 2, W // 2), gen, -2, 2, 0.5)
    w = torch.zeros(Cout, 3, 7, 7, requires_grad=True)   # the weights play no part in their own gradient
    y = F.conv2d(x, w, stride=2, padding=3)
    assert tuple(y.shape) == tuple(d.shape)
    y.backward(d)
    return x, d.permute(0, 2, 3, 1).contiguous().to(bf16), w.grad.permute(0, 2, 3, 1).contiguous()


def run_stem_wgrad(x, d_raw0, Cout):
    _lib, L = _lib_dbg()
    N, _, H, W = x.shape
    assert d_raw0.dtype == bf16 and tuple(d_raw0.shape) == (N, H // 2, W // 2, Cout)
    dw = torch.full((Cout, 7, 7, 3), float("nan"), device=x.device)
    _lib.check(L.dali_debug_stem_wgrad(_lib.ctx(x.device), _lib.stream_ptr(), _lib.ptr(x, torch.float32), _lib.ptr(d_raw0, bf16), N, H, W, Cout,
                                       _lib.ptr(dw)), "dali_debug_stem_wgrad")
    return dw


@pytest.mark.parametrize("case", STEM_CASES)
def test_stem_wgrad_exact_integers(ops_nn, case):
    N, H, W, Cout = case
    _lib, L = _lib_dbg()
    P = N * (H // 2) * (W // 2)
    sp, pps, last = stem_splits(L, Cout, P)
    if case == (2, 32, 32, 32) or case == (3, 64, 32, 64):
        assert P < 16384 and sp > 1                      # the 128 x 128 kernel (two n tiles: 128 + 96 columns), more than one slab
    elif case == (2, 256, 128, 64):
        assert P == 16384 and sp > 1 and last == pps     # exactly the threshold of the 128 x 256 branch, whole splits
    elif case == (43, 32, 48, 64):
        wo, hw = W // 2, (H // 2) * (W // 2)
        assert P > 16384 and (wo & (wo - 1)) and (hw & (hw - 1))        # lw = lhw = -1: the division path of the pixel decomposition
        assert 2 * last == pps, (sp, pps, last)          # the last split holds half the pixels of the others
    else:
        assert sp == L.dali_debug_wgrad_splits(Cout, 224, 2097152, 7, 0), sp       # the split count of batch 256 at 256 x 128
    x, d, ref = stem_case(case)
    xg, dg = x.cuda(), d.cuda()
    dw = run_stem_wgrad(xg, dg, Cout)
    assert torch.equal(dw.cpu(), ref), (case, sp, float((dw.cpu() - ref).abs().max()))
    again = run_stem_wgrad(xg, dg, Cout)
    assert torch.equal(bits32(dw), bits32(again))        # bit-reproducible


def plant_ties(w, count=12):
    """Overwrites `count` elements of the contiguous fp32 tensor w with values whose low 16 bits are exactly 0x8000 -- halfway between two bf16
    values -- with even and odd upper halves in turn, and checks that torch's CPU cast rounds them to nearest even (the expectation's own rule)."""
    flat = w.view(-1)
    raw = flat.view(torch.int32)
    idx = torch.linspace(0, flat.numel() - 1, count).long().unique().tolist()
    want = []
    for j, e in enumerate(idx):
        upper = (((int(raw[e]) & 0xffffffff) >> 16) & ~1) | (j & 1)
        v = (upper << 16) | 0x8000
        raw[e] = v - (1 << 32) if v >= (1 << 31) else v
        want.append((upper + (upper & 1)) & 0xffff)      # ties to even: an odd upper half rounds up, an even one down
    got = [int(b) & 0xffff for b in bits16(flat.to(bf16))[idx]]
    assert got == want and torch.isfinite(flat[idx]).all()
    return w


def random_oracle_net(layers, width, seed):
    """the CPU reference module with random fp32 conv weights (bf16 ties planted in every one), random gamma / beta, random running means and
    running variances in [0.25, 4]"""
    torch.manual_seed(seed)
    ref = OracleNet(layers=layers, width=width)
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, torch.nn.Conv2d):
                o, i, r, s = m.weight.shape
                m.weight.copy_(plant_ties((torch.randn(o, i, r, s, generator=g) * (2.0 / (o * r * s)) ** 0.5).contiguous()))
            elif isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)):
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.5 * torch.randn(m.running_mean.shape, generator=g))
                m.running_var.copy_(0.25 + 3.75 * torch.rand(m.running_var.shape, generator=g))
    return ref


def plan_net(ref, layers, width):
    from daliid_amd import Encoders
    net = Encoders.ResNet50ReID(layers=layers, width=width)
    net.load_state_dict(ref.state_dict())
    return net


def test_stem_packing_bit_patterns(ops_nn):
    """ximg = the image cast to bf16 inside a 3-pixel zero border, 2 further zero columns on the right, a zero 4th channel; w_stem = conv1.weight in
    OHWI cast to bf16 (round to nearest even: planted ties) with a zero tap s = 7 and a zero channel 3"""
    layers, width, (N, H, W) = (1, 1, 1, 1), 32, (2, 64, 32)
    ref = random_oracle_net(layers, width, 11)
    net = plan_net(ref, layers, width)
    x = torch.randn(N, 3, H, W, generator=torch.Generator().manual_seed(12))
    net.eval()
    net._run_forward(x.cuda(), training=False)
    want_x = torch.zeros(N, H + 6, W + 8, 4, dtype=bf16)
    want_x[:, 3:3 + H, 3:3 + W, :3] = x.permute(0, 2, 3, 1).to(bf16)
    got_x = net.debug_tensor("ximg", bf16, (N, H + 6, W + 8, 4)).cpu()
    assert torch.equal(bits16(got_x), bits16(want_x))
    want_w = torch.zeros(width, 7, 8, 4, dtype=bf16)
    want_w[:, :, :7, :3] = ref.conv1.weight.detach().permute(0, 2, 3, 1).to(bf16)
    got_w = net.debug_tensor("w_stem", bf16, (width, 7, 8, 4)).cpu()
    assert torch.equal(bits16(got_w), bits16(want_w))


def test_plan_stem_wgrad_is_the_debug_entry(ops_nn):
    """wiring: after a training forward and backward the plan's conv1.weight gradient equals dali_debug_stem_wgrad on the same images and the plan's
    own d_raw0, bit for bit (same kernels, same split plan)"""
    layers, width, (N, H, W) = (1, 1, 1, 1), 64, (8, 256, 128)
    ref = random_oracle_net(layers, width, 21)
    net = plan_net(ref, layers, width)
    g = torch.Generator().manual_seed(22)
    x = torch.randn(N, 3, H, W, generator=g).cuda()
    d_emb = torch.randn(N, width * 32, generator=g).cuda()
    net.train()
    net._run_forward(x, training=True)
    for stage in range(4):
        net._backward_stage(d_emb, stage)
    d_raw0 = net.debug_tensor("d_raw0", bf16, (N, H // 2, W // 2, width))
    got = net._grad_views["conv1.weight"].permute(0, 2, 3, 1).contiguous()      # logical OIHW -> the stored OHWI
    assert float(d_raw0.float().abs().max()) > 0 and float(got.abs().max()) > 0
    want = run_stem_wgrad(x, d_raw0, width)
    assert torch.equal(bits32(got), bits32(want)), float((got - want).abs().max())


# ---- 2. weight images through the plan ------------------------------------------------------------------------------------------------------
def sqrt_f32(x):
    """The IEEE (correctly rounded) fp32 square root: numpy's fp64 square root -- the hardware instruction -- rounded once more to fp32; 53 bits
    >= 2 * 24 + 2 make that double rounding innocuous.  torch.sqrt on the CPU is NOT the reference here: its vector-library form differs from the
    correctly rounded result in the last bit of 0.6 % of fp32 inputs in [0.25, 4] (and of fp64 ones), which is how this test first failed, while the
    kernel's sqrtf / division compile to the correctly rounded sequences."""
    assert x.dtype == torch.float32
    return torch.from_numpy(np.sqrt(x.numpy().astype(np.float64)).astype(np.float32))


def bn_eval_coeffs(m):
    """scale = gamma / sqrt(rv + eps), shift = beta - rm * scale: fp32, one correctly rounded operation at a time, in the kernel's order"""
    scale = m.weight.detach() / sqrt_f32(m.running_var + torch.tensor(1e-5, dtype=torch.float32))
    return scale, m.bias.detach() - m.running_mean * scale


def weight_image_expectations(ref):
    """name -> expected tensor, for every conv and every BatchNorm in front of the head: the plan's debug-tensor names"""
    exp = {}
    exp["bn1.scale"], exp["bn1.shift"] = bn_eval_coeffs(ref.bn1)
    blocks = [b for l in (ref.layer1, ref.layer2, ref.layer3, ref.layer4) for b in l]
    n_conv = 0
    for i, blk in enumerate(blocks):
        convs, bns = {"1": blk.conv1, "2": blk.conv2, "3": blk.conv3}, {"1": blk.bn1, "2": blk.bn2, "3": blk.bn3}
        if blk.downsample is not None:
            convs["d"], bns["d"] = blk.downsample[0], blk.downsample[1]
        for k, c in convs.items():
            w = c.weight.detach().permute(0, 2, 3, 1).contiguous().to(bf16)          # [cout][r][s][cin]
            exp["block%d.conv%s.w" % (i, k)] = w
            exp["block%d.conv%s.wt" % (i, k)] = w.permute(3, 1, 2, 0).contiguous()   # [cin][r*s][cout]
            n_conv += 1
        for k, m in bns.items():
            exp["block%d.bn%s.scale" % (i, k)], exp["block%d.bn%s.shift" % (i, k)] = bn_eval_coeffs(m)
    return exp, n_conv, n_conv + 1                                                   # transposes, BatchNorm coefficient jobs (+ the stem's)


# (layers, width, more than one 56-job chunk?): the general 32-tile transpose in one chunk; the 64-tile transpose and the general one in two chunks
# (ResNet-50 has 52 transposes and 53 BatchNorms: one chunk; (1, 1, 18, 1) has 67 and 68, the shape of ResNet-101's layer3 cut to 18 blocks)
WEIGHT_NETS = [((1, 1, 1, 1), 32, False), ((1, 1, 18, 1), 64, True), ((1, 1, 18, 1), 32, True)]


@pytest.mark.parametrize("layers,width,two_chunks", WEIGHT_NETS)
def test_weight_images_and_eval_coefficients_bit_for_bit(ops_nn, layers, width, two_chunks):
    """Every conv's bf16 image and its transpose, every BatchNorm's eval scale / shift, after one eval forward.
    scale: IEEE division and square root are correctly rounded, so a correctly rounded fp32 evaluation on the CPU (sqrt_f32 above) is the
    expectation, bit for bit; measured on an MI355X: no element of any scale or shift vector differs."""
    ref = random_oracle_net(layers, width, 31 + width + sum(layers))
    exp, n_tr, n_bn = weight_image_expectations(ref)
    if two_chunks:
        assert n_tr > 56 and n_bn > 56, (n_tr, n_bn)     # the launchers' second-chunk loops run
    else:
        assert n_tr <= 56 and n_bn <= 56
    net = plan_net(ref, layers, width)
    net.eval()
    x = torch.randn(2, 3, 64, 32, generator=torch.Generator().manual_seed(5))
    net._run_forward(x.cuda(), training=False)
    bad = []
    for name, want in exp.items():
        got = net.debug_tensor(name, want.dtype, tuple(want.shape)).cpu()
        same = torch.equal(bits16(got), bits16(want)) if want.dtype == bf16 else torch.equal(bits32(got), bits32(want))
        if not same:
            bad.append((name, int((got != want).sum())))
    assert not bad, (len(bad), bad[:8])


def test_folded_hi_lo_weight_image(ops_nn):
    """the inference forward's [W3 hi | W3 lo | Wd hi | Wd lo] image and summed shift of layer1's first block, from the plan's own BatchNorm
    coefficients and the fp32 master weights: v = s[c] * w[c][col], hi = bf16(v), lo = bf16(v - float(hi))"""
    layers, width = (1, 1, 1, 1), 64
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n_cus = cus & ~7 if cus > 8 else 8
    # conv_cat_act_supported(256, 64, 64, P, 2): the persistent kernel wants 2 tiles of 128 x 128 per CU (2 channel tiles x P / 128 pixel tiles)
    # and channel tiles that divide an XCD's CUs.  P = N * 64 * 32 at 256 x 128 images: N = 16 on 256 CUs
    N = -(-128 * n_cus // (64 * 32))
    ref = random_oracle_net(layers, width, 41)
    net = plan_net(ref, layers, width)
    net.eval()
    x = torch.randn(N, 3, 256, 128, generator=torch.Generator().manual_seed(6))
    net._run_forward(x.cuda(), training=False)
    C, w, cin = 4 * width, width, width
    wcat = net.debug_tensor("block0.wcat", bf16, (C, 2 * (w + cin))).cpu()           # raises if this plan does not fold the block
    shcat = net.debug_tensor("block0.shcat", torch.float32, (C,)).cpu()
    s3, h3, sd, hd = (net.debug_tensor("block0.bn%s.%s" % (b, f), torch.float32, (C,)).cpu() for b in "3d" for f in ("scale", "shift"))
    blk = ref.layer1[0]
    parts = []
    for s, conv in ((s3, blk.conv3), (sd, blk.downsample[0])):
        v = s[:, None] * conv.weight.detach().reshape(C, -1)                         # 1x1: [C][cin]
        hi = v.to(bf16)
        lo = (v - hi.float()).to(bf16)
        assert int((bits16(lo) != 0).sum()) > lo.numel() // 2                        # the low part is exercised
        parts += [hi, lo]
    want = torch.cat(parts, dim=1)
    assert torch.equal(bits16(wcat), bits16(want)), int((bits16(wcat) != bits16(want)).sum())
    assert torch.equal(bits32(shcat), bits32(h3 + hd))


# ---- 3. masked head-pool backward -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["both", "gap", "gmp"])
@pytest.mark.parametrize("n,h,w,C", [(3, 16, 8, 2048), (5, 4, 2, 1024), (2, 6, 3, 64)])      # the plan's head; small; HW = 18: the division path
def test_head_pool_bwd_masked(ops_nn, n, h, w, C, mode):
    _lib, L = _lib_dbg()
    g = torch.Generator().manual_seed(n * 100 + h + C)
    x = torch.randn(n, h, w, C, generator=g).to(bf16).cuda()
    df = torch.randn(n, C, generator=g).cuda()
    keep = (torch.rand(n, h, w, C, generator=g) < 0.5).cuda()
    assert 0.2 < float(keep.float().mean()) < 0.8
    _, arg = ops_nn.head_pool_fwd(x, mode)
    plain = ops_nn.head_pool_bwd(df, arg, (h, w), mode)
    want = torch.where(keep, plain, torch.zeros_like(plain))
    dx = torch.full((n, h, w, C), float("nan"), device="cuda", dtype=bf16)
    _lib.check(L.dali_debug_head_pool_bwd_masked(_lib.ctx(df.device), _lib.stream_ptr(), _lib.ptr(df, torch.float32), _lib.ptr(arg), n, h * w, C,
                                                 ops_nn.FEATURE_MODES[mode], _lib.ptr(bits_of(keep)), _lib.ptr(dx)), "dali_debug_head_pool_bwd_masked")
    assert float(plain.float().abs().max()) > 0
    assert torch.equal(bits16(dx), bits16(want)), int((bits16(dx) != bits16(want)).sum())


# ---- 4. column sums riding on the weight-gradient GEMMs -------------------------------------------------------------------------------------
def colsum_inputs(P, C, w, dev):
    assert 9 * P < 2 ** 24                               # a in [0, 3]: Gram entries <= 9 P; |dz| <= 2: every partial sum exact in fp32, in any order
    g = torch.Generator().manual_seed(P + C + w)
    a = ints((P, w), g, 0, 3).to(dev)
    W = (torch.randn(C, w, generator=g) / w ** 0.5).to(bf16).to(dev)
    gamma, beta = (0.5 + torch.rand(C, generator=g)).to(dev), (0.2 * torch.randn(C, generator=g)).to(dev)
    return g, a, W, gamma, beta


def gram_reference(a):
    ad = a.double()
    return (ad.T @ ad).float(), ad.sum(0).float()        # integers below 2^24: the fp64 results are exact and convert exactly


# the 128 x 128 kernel, one column-sum row per split, ragged P; the pipelined 128 x 256 kernel with 1, 2 and 3 k-steps in its last split; a
# 5-pixel last k-step with two n tiles (rows per (split, n tile)) and three m tiles; the plan's layer4 shape
COLSUM_CASES = [(2048, 128, 32), (4100, 256, 64), (16416, 1024, 256), (16448, 1024, 256), (16480, 1024, 256), (16421, 384, 512), (32768, 2048, 512)]


@pytest.mark.parametrize("P,C,w", COLSUM_CASES)
def test_gemm_column_sums_exact_integers(ops_nn, P, C, w):
    g, a, W, gamma, beta = colsum_inputs(P, C, w, "cuda")
    ref_gram, ref_m2 = gram_reference(a)
    ab = a.to(bf16)
    o = ops_nn.bnlin_fwd(ab, W, gamma, beta)
    assert torch.equal(o["m2"], ref_m2), float((o["m2"] - ref_m2).abs().max())
    assert torch.equal(o["gram"], ref_gram), float((o["gram"] - ref_gram).abs().max())
    dz = ints((P, C), g, -2, 2, 0.5).cuda()
    ob = ops_nn.bnlin_bwd(dz.to(bf16), ab, W, o)
    ref_db = dz.double().sum(0).float()
    assert torch.equal(ob["dbeta"], ref_db), float((ob["dbeta"] - ref_db).abs().max())      # the row kernel stores s_dz = colsum(dz) unchanged


def test_gram_column_sums_two_workgroup_kernel(ops_nn):
    """WG_WG[1] (see the module docstring): the smallest Gram GEMM with more than 100 tiles of 128 x 256, eight n tiles sharing the column sums"""
    P, C, w = 16384, 32, 1824
    assert -(-w // 128) * -(-w // 256) > 100 and -(-(w - 32) // 128) * -(-(w - 32) // 256) <= 100
    g, a, W, gamma, beta = colsum_inputs(P, C, w, "cuda")
    ref_gram, ref_m2 = gram_reference(a)
    o = ops_nn.bnlin_fwd(a.to(bf16), W, gamma, beta)
    assert torch.equal(o["m2"], ref_m2), float((o["m2"] - ref_m2).abs().max())
    assert torch.equal(o["gram"], ref_gram), float((o["gram"] - ref_gram).abs().max())
