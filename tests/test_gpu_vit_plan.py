"""The ViT plan's WIRING (daliid_amd/csrc/vit_plan.hip), op by op and block by block, from the plan's own tensors.

Every ViT kernel is held tightly on its own (tests/test_gpu_vit_plan_shapes.py, test_gpu_vit_ops.py, test_gpu_nnops_plan_sizes.py); how the plan
strings them together was checked only by the whole-net comparisons of tests/test_gpu_vit.py (2e-2 .. 0.15), inside which a wrong operand, a
neighbour's DropPath factor or a bias gradient short of a few rows fits (tests/test_vit_twin_cpu.py measures by how much).  Here:

 (a) forward: every stored output against its op applied in fp64 to the plan's own stored inputs and the fp32 master parameters (weights as
     P.to(bf16)), within bounds derived next to each assertion;
 (b) the pieces without a single-op entry point, bit for bit: DropPath rows, the bf16 weight image, the batched transposes (60 jobs = two chunks),
     the cls-row gather, memset + scatter, the token tail's copy; the final-norm backward (fp32 upstream gradient) and the neck backward without
     dbeta against fp64; which gradient slots the backward writes at all (NaN sentinel);
 (c) backward, block by block (dali_debug_vit_backward_block): each block's d x_in and 12 parameter gradients against the rounding-matched twin
     (oracle/vit_bf16.py) fed the plan's own stored tensors and incoming gradient, so that errors do not chain; the token tail exactly;
 (d) dali_vit_backward == the stages one by one == the debug calls, bit for bit; a stage's parameter range is final once the stage has run.

Nets (all ViTNeckNet in train mode, perturbed weights, non-trivial affines):
  A  64 x 32, 9 tokens, B 6 (54 rows, less than one attention tile), dim 128, depth 4, no DropPath
  B  256 x 128 at stride 12, 211 tokens, B 4 (844 rows), dim 128, depth 3, DropPath 0.5 with injected draws
  C  224 x 224, 197 tokens, B 2, ViT-B widths (dim 768: the NCH = 2 LayerNorm, linears of N = 2304 / 3072), depth 2, DropPath 0.1
  D  as A at depth 6: backward stages of 1, 2, 1 and 2 blocks
"""
import ctypes
import functools
import time
import types

import numpy as np
import pytest
import torch

from oracle import vit_bf16 as TW
from vit_checks import U, HB, assert_within, check_bn1d_bwd, check_layernorm_fwd, ulp32

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
U1 = 2.0 ** -23
LN_EPS = float(np.float32(1e-6))
BN_EPS = float(np.float32(1e-5))
SENTINEL = 0x7FC0BEEF               # a quiet NaN with a recognisable payload, as int32
DALI_ERR_INVALID = -1               # include/daliid.h

# ---- bounds of (c): HIP against the twin, rel-L2 per quantity family.  They cannot be derived: the twin sums in another order, a difference in the
# last fp32 bit flips some bf16 roundings, and every further bf16 store of the chain (eight per block) turns a relative difference d of its input
# into about sqrt(d * 2^-8) of flipped roundings, so the figure depends on the data and grows with the width (longer sums seed more flips, and at
# dim 768 the branches outweigh the residual).  Each bound is 2x the largest value measured on an MI355X over nets A, B, C (docs/experiments.md,
# "ViT plan, block by block"), the margin of tests/test_gpu_resnet_blocks.py; no test was failing in the measuring run.
#                        measured maxima:   net A       net B       net C
BOUND_DX = 5.58e-3      # d x_in            4.998e-05   3.879e-04   2.788e-03
BOUND_LN = 4.31e-3      # LayerNorm grads   2.444e-04   1.195e-03   2.155e-03
BOUND_W = 3.11e-3       # weight grads      8.194e-05   7.023e-04   1.553e-03
BOUND_B = 4.00e-3       # bias grads        2.146e-04   1.281e-03   2.000e-03
# (with other DropPath draws -- both branches of a block dropping the same sample -- the same nets gave 3.05e-3, 2.48e-3, 2.05e-3 and 2.37e-3
# on net C and 5.8e-6 .. 1.9e-4 on net B: which roundings flip depends on the data)

NETS = {
    "A": dict(img=(64, 32), stride=16, B=6, dim=128, heads=2, depth=4, rate=0.0),
    "B": dict(img=(256, 128), stride=12, B=4, dim=128, heads=2, depth=3, rate=0.5),
    "C": dict(img=(224, 224), stride=16, B=2, dim=768, heads=12, depth=2, rate=0.1),
    "D": dict(img=(64, 32), stride=16, B=6, dim=128, heads=2, depth=6, rate=0.0),
}
LINS = (("qkv", "attn.qkv"), ("proj", "attn.proj"), ("fc1", "mlp.fc1"), ("fc2", "mlp.fc2"))
BLOCK_TENSORS = ("h1", "qkv", "att", "x_mid", "h2", "pre1", "act1", "x_out")
BLOCK_STATS = ("lse", "n1.mean", "n1.rstd", "n2.mean", "n2.rstd")


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == bf16 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


def halfulp_bf16(a):
    """half a bf16 ulp at magnitude |a| (float64)"""
    _, e = torch.frexp(a.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(a), e.to(a.dtype) - 9)


@functools.lru_cache(maxsize=None)
def _dbg():
    """the diagnostic entry points (include/daliid_debug.h), bound here: nothing under daliid_amd/ binds them"""
    from daliid_amd import _lib
    L = _lib.lib()
    vp = ctypes.c_void_p
    L.dali_debug_vit_tensor.argtypes = [vp, ctypes.c_char_p, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_int64)]
    L.dali_debug_vit_backward_block.argtypes = [vp, vp, vp, ctypes.c_int]
    return _lib, L


class Plan:
    """a ViTNeckNet with its last plan's arena tensors by name"""

    def __init__(self, net, cfg):
        self.net, self.cfg = net, cfg
        self.B, self.C, self.H, self.depth = cfg["B"], cfg["dim"], cfg["heads"], cfg["depth"]
        self.T = net.base.pos_embed.shape[1]
        self.rows, self.Hd = self.B * self.T, 4 * cfg["dim"]
        self.table = {name: (off, numel, shape) for name, off, numel, shape in net._plan(self.B).tensor_table(0)}

    def view(self, name, dtype):
        """the arena bytes of a named tensor, in place"""
        _lib, L = _dbg()
        ptr, nbytes = ctypes.c_void_p(), ctypes.c_int64()
        _lib.check(L.dali_debug_vit_tensor(self.net._last_plan.h, name.encode(), ctypes.byref(ptr), ctypes.byref(nbytes)), "dali_debug_vit_tensor " + name)
        off = ptr.value - self.net._arena.data_ptr()
        assert 0 <= off and off + nbytes.value <= self.net._arena.numel(), name
        return self.net._arena[off:off + nbytes.value].view(dtype)

    def get(self, name, dtype, *shape):
        torch.cuda.synchronize()
        return self.view(name, dtype).view(*shape).cpu()

    def status(self, name):
        _lib, L = _dbg()
        ptr, nbytes = ctypes.c_void_p(), ctypes.c_int64()
        return L.dali_debug_vit_tensor(self.net._last_plan.h, name.encode(), ctypes.byref(ptr), ctypes.byref(nbytes))

    def bwd(self, d_feat, block):
        _lib, L = _dbg()
        _lib.check(L.dali_debug_vit_backward_block(self.net._last_plan.h, _lib.stream_ptr(), _lib.ptr(d_feat), block), "dali_debug_vit_backward_block")

    def param(self, name):
        """fp32 master parameter on the host"""
        off, numel, shape = self.table[name]
        return self.net.flat_params[off:off + numel].view(*shape).detach().cpu()

    def grad(self, flat, name):
        off, numel, shape = self.table[name]
        return flat[off:off + numel].view(*shape)

    def forward_tensors(self):
        rows, C, Hd = self.rows, self.C, self.Hd
        t = {"patches": self.get("patches", bf16, self.B * (self.T - 1), -1), "pe": self.get("pe", bf16, -1, C), "x0": self.get("x0", bf16, rows, C),
             "cls_rows": self.get("cls_rows", bf16, self.B, C), "gf": self.get("gf", torch.float32, self.B, C),
             "fin.mean": self.get("fin.mean", torch.float32, self.B), "fin.rstd": self.get("fin.rstd", torch.float32, self.B),
             "neck.mean": self.get("neck.mean", torch.float32, C), "neck.invstd": self.get("neck.invstd", torch.float32, C)}
        width = {"qkv": 3 * C, "pre1": Hd, "act1": Hd}
        for i in range(self.depth):
            for k in BLOCK_TENSORS:
                t["block%d.%s" % (i, k)] = self.get("block%d.%s" % (i, k), bf16, rows, width.get(k, C))
            t["block%d.lse" % i] = self.get("block%d.lse" % i, torch.float32, self.B * self.H, self.T)
            for k in BLOCK_STATS[1:]:
                t["block%d.%s" % (i, k)] = self.get("block%d.%s" % (i, k), torch.float32, rows)
        return t


def make_net(cfg, seed=3):
    from daliid_amd import vit_pytorch as V
    net = V.ViTNeckNet(img_size=cfg["img"], patch_size=16, stride_size=cfg["stride"], embed_dim=cfg["dim"], depth=cfg["depth"], num_heads=cfg["heads"],
                       mlp_ratio=4.0, num_classes=10, drop_path_rate=cfg["rate"], seed=seed)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for p in net.parameters():                       # as test_small_vit_forward_backward_vs_oracle: LayerNorm and neck affines end up non-trivial
            p.add_((0.05 * torch.randn(p.shape, generator=g)).to(p.device))
    net.mark_weights_changed()
    net.train()
    return net, g


def injected_draws(cfg, g):
    """uniform draws [2*depth, B]: in every branch of the blocks with a non-zero rate one of samples 0 and 1 is dropped and the other kept, the
    attention branch dropping sample 0 and the MLP branch sample 1 (so that no two branches of a block share their factors, at B = 2 either)"""
    u = torch.rand(2 * cfg["depth"], cfg["B"], generator=g)
    lo, hi = 0.0005, 0.9995                              # floor(keep + u) = 0 for every keep < 0.9995, 1 for every keep > 0.0005
    u[0::2, 0], u[0::2, 1] = lo, hi
    u[1::2, 0], u[1::2, 1] = hi, lo
    return u


def nan_fill(net):
    bits(net.flat_grads).fill_(SENTINEL)


@functools.lru_cache(maxsize=None)
def run(name):
    """one forward and one block-by-block backward of net `name`; everything the tests of (a), (b), (c) read, on the host"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    t0 = time.time()
    cfg = NETS[name]
    net, g = make_net(cfg)
    P = Plan(net, cfg)
    x = torch.randn(cfg["B"], 3, *cfg["img"], generator=g)
    d_feat = torch.randn(cfg["B"], cfg["dim"], generator=g)
    if cfg["rate"] > 0:
        net.drop_path_uniform = injected_draws(cfg, g).cuda()
    r = types.SimpleNamespace(P=P, net=net, cfg=cfg, x=x, d_feat=d_feat)
    r.feat = net._run_forward(x.cuda(), True).cpu()
    r.scales = net._dp_scales.cpu() if net._dp_scales is not None else None
    r.t = P.forward_tensors()
    r.dp_rows = P.get("dp_rows", torch.float32, 2 * P.depth, P.rows) if r.scales is not None else None
    r.wbf16 = P.get("wbf16", bf16, -1)
    # backward, one piece at a time
    nan_fill(net)
    dg = d_feat.cuda()
    P.bwd(dg, P.depth)
    r.after_head = dict(grad_cur=P.get("grad_cur", bf16, P.B, P.T, P.C), dcls_rows=P.get("dcls_rows", bf16, P.B, P.C),
                        dgf=P.get("dgf", torch.float32, P.B, P.C), flat=net.flat_grads.cpu())
    r.d_in = {P.depth - 1: r.after_head["grad_cur"].reshape(P.rows, P.C)}       # gradient ENTERING block i (= d x_out of block i)
    for i in range(P.depth - 1, -1, -1):
        P.bwd(dg, i)
        r.d_in[i - 1] = P.get("grad_cur", bf16, P.rows, P.C)                    # d_in[-1]: the gradient entering the token tail
    P.bwd(dg, -1)
    r.dpe = P.get("dpe", bf16, P.B, P.T - 1, P.C)
    r.grad_cur_after_tail = P.get("grad_cur", bf16, P.B, P.T, P.C)
    r.flat = net.flat_grads.cpu()
    torch.cuda.synchronize()
    print("\nnet %s: forward + block-by-block backward + read-back %.1f s" % (name, time.time() - t0))
    return r


def lin_ref(x, w, bias):
    """fp64 x w^T + bias on bf16 operands, and the fp32 accumulation bound (K + 2) 2^-23 (|x| |w|^T + |bias|): K products summed in any order
    inside the MFMAs and across k-tiles (<= K roundings of partial sums bounded by the sum of magnitudes), the bias add, one spare"""
    xd, wd, bd = x.double(), w.double(), bias.double()
    acc = xd @ wd.t() + bd
    E = (x.shape[1] + 2) * U1 * (xd.abs() @ wd.abs().t() + bd.abs())
    return acc, E


def check_stored(got, ref, E, what):
    """a bf16 store of an fp32 value within E of ref: half a bf16 ulp at |ref| + E, plus E"""
    assert_within(got.double(), ref, halfulp_bf16(ref.abs() + E) + E, what)


# ---------------------------------------------------------------------------------------------------------------------------------------
# (a) forward, op by op
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_forward_op_by_op(name):
    from test_gpu_nnops_plan_sizes import _bn1d_check_y
    from test_gpu_vit_plan_shapes import _check_attention, _gelu_bound, _phi_Phi
    from daliid_amd import ops_vit
    r = run(name)
    P, t = r.P, r.t
    B, T, C, H, rows = P.B, P.T, P.C, P.H, P.rows
    W = lambda k: P.param(k).to(bf16)                                            # the plan's weight image (checked bit for bit in (b))
    # tokens: pe = patches Wp^T + b stored once; x0 = (cls | pe) + pos: one fp32 add of exact operands, one rounding -> bit for bit
    acc, E = lin_ref(t["patches"], W("base.patch_embed.proj.weight").reshape(C, -1), P.param("base.patch_embed.proj.bias"))
    check_stored(t["pe"], acc, E, "pe")
    x0 = (torch.cat((P.param("base.cls_token").reshape(1, 1, C).expand(B, 1, C), t["pe"].float().reshape(B, T - 1, C)), 1)
          + P.param("base.pos_embed").reshape(1, T, C)).reshape(rows, C).to(bf16)
    assert same_bits(t["x0"], x0), "x0"
    if r.scales is not None:
        assert same_bits(r.dp_rows, r.scales.repeat_interleave(T, dim=1)), "dp_rows"         # the factors used below are the caller's
    x_in = t["x0"]
    g_att = torch.Generator().manual_seed(7)
    for i in range(P.depth):
        pre = "base.blocks.%d." % i
        b = lambda k: t["block%d.%s" % (i, k)]
        prm = lambda k: P.param(pre + k)
        what = "net %s block %d " % (name, i)
        # LayerNorm 1: the bound of test_layernorm_fwd_vit_plan_size (tests/vit_checks.py)
        check_layernorm_fwd(b("h1"), b("n1.mean"), b("n1.rstd"), x_in, prm("norm1.weight"), prm("norm1.bias"), LN_EPS, what + "LN1")
        # qkv = h1 Wqkv^T + bias: half a bf16 ulp + the fp32 accumulation bound
        acc, E = lin_ref(b("h1"), W(pre + "attn.qkv.weight"), prm("attn.qkv.bias"))
        check_stored(b("qkv"), acc, E, what + "qkv")
        # attention on the plan's own qkv: output and lse by _check_attention's derived bounds (its backward part runs the single-op kernel on the
        # plan's own qkv / att / lse and a random d_out)
        d_o = torch.randn(rows, C, generator=g_att).to(bf16)
        dqkv = ops_vit.attention_bwd(b("qkv").cuda(), b("att").cuda(), d_o.cuda(), b("lse").cuda(), B, T, H)
        _check_attention(b("qkv"), d_o, b("att"), b("lse"), dqkv.cpu(), B, T, H, what + "attention")
        # x_mid = x_in + s (att Wproj^T + bias) in the documented order ((acc + bias) x s) + res: the accumulation bound scaled by |s|, one
        # rounding of the product and one of the sum (<= 2^-23 of their magnitudes), then bf16
        s = r.dp_rows[2 * i].double().unsqueeze(1) if r.scales is not None else torch.ones(rows, 1, dtype=torch.float64)
        acc, E = lin_ref(b("att"), W(pre + "attn.proj.weight"), prm("attn.proj.bias"))
        ref = x_in.double() + s * acc
        check_stored(b("x_mid"), ref, s.abs() * E + U1 * ((s * acc).abs() + ref.abs()), what + "x_mid")
        check_layernorm_fwd(b("h2"), b("n2.mean"), b("n2.rstd"), b("x_mid"), prm("norm2.weight"), prm("norm2.bias"), LN_EPS, what + "LN2")
        # pre1 = h2 W1^T + bias stored once; act1 = GELU of the SAME fp32 accumulator: _gelu_bound at the fp64 accumulator reference, plus the
        # accumulator's own error E through |GELU'| <= 1.13
        acc, E = lin_ref(b("h2"), W(pre + "mlp.fc1.weight"), prm("mlp.fc1.bias"))
        check_stored(b("pre1"), acc, E, what + "pre1")
        gref = acc * _phi_Phi(acc)[1]
        assert_within(b("act1").double(), gref, _gelu_bound(acc, gref) + 1.13 * (1 + HB) * E, what + "act1")
        s = r.dp_rows[2 * i + 1].double().unsqueeze(1) if r.scales is not None else torch.ones(rows, 1, dtype=torch.float64)
        acc, E = lin_ref(b("act1"), W(pre + "mlp.fc2.weight"), prm("mlp.fc2.bias"))
        ref = b("x_mid").double() + s * acc
        check_stored(b("x_out"), ref, s.abs() * E + U1 * ((s * acc).abs() + ref.abs()), what + "x_out")
        x_in = b("x_out")
    # head: the strided cls-row gather, the final LayerNorm's fp32 output (no bf16 term), the neck in training mode
    assert same_bits(t["cls_rows"], x_in.reshape(B, T, C)[:, 0].contiguous()), "cls_rows"
    check_layernorm_fwd(t["gf"], t["fin.mean"], t["fin.rstd"], t["cls_rows"], P.param("base.norm.weight"), P.param("base.norm.bias"), LN_EPS,
                        "final LayerNorm (fp32 output)", y_bf16=False)
    gd = t["gf"].double()
    m64 = gd.mean(0)
    i64 = 1.0 / torch.sqrt(((gd - m64) ** 2).sum(0) / B + BN_EPS)
    assert_within(t["neck.mean"].double(), m64, torch.from_numpy(ulp32(m64.numpy())), "neck mean")           # as test_bn1d_train_plan_sizes
    assert_within(t["neck.invstd"].double(), i64, torch.from_numpy(ulp32(i64.numpy())), "neck invstd")
    _bn1d_check_y(r.feat, t["gf"], m64, i64, P.param("bottleneck.weight"), P.param("bottleneck.bias"), "neck output")


def test_rate0_forward_never_reads_dp_rows():
    """net A has no DropPath: run_block gets null factor pointers.  Asserted through the values: with dp_rows poisoned (NaN) a second forward
    stores the same bits everywhere"""
    r = run("A")
    P = r.P
    assert r.net._dp_scales is None
    bits(P.view("dp_rows", torch.float32)).fill_(SENTINEL)
    feat = r.net._run_forward(r.x.cuda(), True).cpu()
    assert same_bits(feat, r.feat)
    t2 = P.forward_tensors()
    for k, v in r.t.items():
        assert same_bits(t2[k], v), k


# ---------------------------------------------------------------------------------------------------------------------------------------
# (b) plan-only pieces, exactly
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["B", "C"])
def test_droppath_rows_and_draws(name):
    r = run(name)
    P = r.P
    assert same_bits(r.dp_rows, r.scales.repeat_interleave(P.T, dim=1))          # dp_rows[j][b*T + t] == scales[j][b]
    first = 1                                                                    # block 0 has rate 0 (vit_pytorch.py:338): factors 1
    assert set(r.scales[:2].flatten().tolist()) == {1.0}
    for j in range(2 * first, 2 * P.depth):
        assert bool((r.scales[j] == 0).any()) and bool((r.scales[j] > 1).any()), "branch %d needs a dropped and a kept sample" % j
    for i in range(first, P.depth):
        assert not torch.equal(r.scales[2 * i], r.scales[2 * i + 1]), "block %d: both branches carry the same factors" % i
        if i + 1 < P.depth:
            assert not torch.equal(r.scales[2 * i], r.scales[2 * i + 2]), "blocks %d and %d: the same attention factors" % (i, i + 1)


@pytest.mark.parametrize("name", ["A", "C"])
def test_weight_image_is_the_cast_of_every_segment(name):
    r = run(name)
    P = r.P
    flat = r.net.flat_params.detach().cpu()
    for k, (off, numel, shape) in P.table.items():
        assert same_bits(r.wbf16[off:off + numel], flat[off:off + numel].to(bf16)), k


def _check_transposes(P, wbf16):
    jobs = 0
    for i in range(P.depth):
        for short, long_ in LINS:
            off, numel, (N, K) = P.table["base.blocks.%d.%s.weight" % (i, long_)]
            w = P.get("block%d.%s.w" % (i, short), bf16, N, K)
            assert same_bits(w, wbf16[off:off + numel].view(N, K)), (i, short, "w is not the image's segment")
            assert same_bits(P.get("block%d.%s.wt" % (i, short), bf16, K, N), w.t().contiguous()), (i, short, "wt")
            jobs += 1
    return jobs


def test_transposed_images_net_c():
    r = run("C")
    assert _check_transposes(r.P, r.wbf16) == 8


def test_transposed_images_60_jobs_two_chunks():
    """depth 15: 60 transpose jobs, four more than one launch of the batched kernel takes (TRANSPOSE_BATCH = 56, nnops.hip)"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    cfg = dict(img=(64, 32), stride=16, B=2, dim=128, heads=2, depth=15, rate=0.0)
    net, g = make_net(cfg)
    net._run_forward(torch.randn(2, 3, 64, 32, generator=g).cuda(), True)
    P = Plan(net, cfg)
    jobs = _check_transposes(P, P.get("wbf16", bf16, -1))
    assert jobs == 60 and jobs > 56


def test_debug_tensor_names():
    r = run("A")
    P = r.P
    for bad in ("nope", "block4.h1", "block-1.h1", "block0.nope", "block0.qkv.nope", "block0.h1x", "blockx"):
        assert P.status(bad) == DALI_ERR_INVALID, bad
    for good in ("patches", "dpe", "grad_cur", "dp_rows", "block3.fc2.wt", "block0.n2.rstd"):
        assert P.status(good) == 0, good
    # an eval-only plan reserves no dgrad images, DropPath rows or gradient buffers
    from daliid_amd import vit_pytorch as V
    ev = V.ViTNeckNet(img_size=(64, 32), patch_size=16, stride_size=16, embed_dim=128, depth=2, num_heads=2, num_classes=10, local_feature=True, seed=1)
    ev.eval()
    ev.local_tokens(torch.zeros(1, 3, 64, 32).cuda())
    Pe = Plan(ev, dict(B=1, dim=128, heads=2, depth=2))
    assert Pe.status("block0.qkv.w") == 0 and Pe.status("x0") == 0
    for k in ("block0.qkv.wt", "dp_rows", "grad_cur", "dpe"):
        assert Pe.status(k) == DALI_ERR_INVALID, k


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_head_backward_scatter_and_sentinels(name):
    """after the head-only call: the token gradient holds dcls_rows at token 0 of every sample and +0 bits elsewhere; of the gradient slots only
    bottleneck.weight and base.norm.* are written (bottleneck.bias is frozen: the neck backward gets a null dbeta)"""
    r = run(name)
    P, h = r.P, r.after_head
    assert same_bits(h["grad_cur"][:, 0].contiguous(), h["dcls_rows"])
    assert int(bits(h["grad_cur"][:, 1:]).count_nonzero()) == 0
    written = torch.zeros(r.flat.numel(), dtype=torch.bool)
    for k in ("bottleneck.weight", "base.norm.weight", "base.norm.bias"):
        off, numel, _ = P.table[k]
        written[off:off + numel] = True
    assert torch.equal(bits(h["flat"]) != SENTINEL, written)
    # after the whole backward.  Today's contract: the backward writes every parameter's gradient exactly once and NEVER touches base.fc.* (the
    # unused head), bottleneck.bias (frozen) or the padding that rounds every segment up to 64 elements; that those read as zero gradients is
    # the allocation's doing (ViTNeckNet.flat_grads = torch.zeros), not the plan's.
    written = torch.zeros(r.flat.numel(), dtype=torch.bool)
    for k, (off, numel, _) in P.table.items():
        if k not in ("base.fc.weight", "base.fc.bias", "bottleneck.bias"):
            written[off:off + numel] = True
    assert torch.equal(bits(r.flat) != SENTINEL, written)
    assert bool(torch.isfinite(r.flat[written]).all())


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_neck_and_final_norm_backward(name):
    """bn1d_bwd with a null dbeta and the LayerNorm backward's fp32-gradient path, against fp64 from the plan's own tensors"""
    r = run(name)
    P, t, h = r.P, r.t, r.after_head
    B, C = P.B, P.C
    gamma_n = P.param("bottleneck.weight")
    check_bn1d_bwd(h["dgf"], P.grad(h["flat"], "bottleneck.weight"), None, t["gf"], r.d_feat, gamma_n, t["neck.mean"].double(), t["neck.invstd"].double(), "neck")
    # LayerNorm backward on B rows from g = dgf (fp32), x = cls_rows, the saved statistics.  test_layernorm_bwd_vit_plan_size bounds the kernel
    # on exact operands by 4u rstd (|g gamma| + |s1| + |xh s2|); with general operands g gamma (1u) and xhat = (x - mean) rstd (2u) round, the
    # row means are sums of C such terms (the forward's 24u for the lane sum and butterfly, + 1u for / C): s1 within 26u mean|g gamma|, s2
    # within 29u mean|g gamma xhat|, and xhat s2 carries xhat's 2u and the product's 1u.  Rounded up: 8u for the terms, 32u for the means.
    g, x = h["dgf"].double(), t["cls_rows"].double()
    mu, rs = t["fin.mean"].double().unsqueeze(1), t["fin.rstd"].double().unsqueeze(1)
    gamma = P.param("base.norm.weight").double()
    xh = (x - mu) * rs
    gh = g * gamma
    s1, s2 = gh.mean(1, keepdim=True), (gh * xh).mean(1, keepdim=True)
    ref = rs * (gh - s1 - xh * s2)
    E = rs * (8 * U * (gh.abs() + s1.abs() + (xh * s2).abs()) + 32 * U * gh.abs().mean(1, keepdim=True) + xh.abs() * 32 * U * (gh * xh).abs().mean(1, keepdim=True))
    assert_within(h["dcls_rows"].double(), ref, HB * ref.abs() + (1 + HB) * E, "final norm d cls_rows")
    # dgamma = sum_b g xhat (3u per term), dbeta = sum_b g: B <= 6 terms through the per-block partials and the finishing reduction (<= B + 2
    # roundings of partial sums bounded by the sum of magnitudes)
    assert_within(P.grad(h["flat"], "base.norm.weight").double(), (g * xh).sum(0), (B + 5) * U * (g * xh).abs().sum(0), "final norm dgamma")
    assert_within(P.grad(h["flat"], "base.norm.bias").double(), g.sum(0), (B + 2) * U * g.abs().sum(0), "final norm dbeta")


# ---------------------------------------------------------------------------------------------------------------------------------------
# (c) backward, block by block, against the rounding-matched twin
# ---------------------------------------------------------------------------------------------------------------------------------------
def block_errors(r):
    """HIP against the twin for every block of a run -> {family: [(what, figure)]}"""
    P, t = r.P, r.t
    C = P.C
    out = {"dx_in": [], "ln": [], "weight": [], "bias": []}
    for i in range(P.depth - 1, -1, -1):
        st = {k: t["block%d.%s" % (i, k)].float() for k in BLOCK_TENSORS + BLOCK_STATS[1:]}
        st["lse"] = t["block%d.lse" % i].reshape(P.B, P.H, P.T)
        st["x_in"] = (t["x0"] if i == 0 else t["block%d.x_out" % (i - 1)]).float()
        prm = {k: P.param("base.blocks.%d.%s" % (i, k)) for k in TW.BLOCK_PARAMS}
        s_att = r.scales[2 * i] if r.scales is not None else None
        s_mlp = r.scales[2 * i + 1] if r.scales is not None else None
        dx, g = TW.backward_block(st, prm, r.d_in[i].float(), P.H, P.B, s_att, s_mlp)
        out["dx_in"].append(("block%d" % i, rel_l2(r.d_in[i - 1].float(), dx)))
        for k in TW.BLOCK_PARAMS:
            got = P.grad(r.flat, "base.blocks.%d.%s" % (i, k))
            what = "block%d.%s" % (i, k)
            if k == "attn.qkv.bias":
                # the k third is zero in exact arithmetic (the rows of dS sum to zero): compared absolutely, on the scale of the q third
                out["bias"].append((what + "[q]", rel_l2(got[:C], g[k][:C])))
                out["bias"].append((what + "[k]", float((got[C:2 * C].double() - g[k][C:2 * C].double()).norm() / g[k][:C].double().norm())))
                out["bias"].append((what + "[v]", rel_l2(got[2 * C:], g[k][2 * C:])))
            else:
                out["ln" if k.startswith("norm") else "bias" if k.endswith(".bias") else "weight"].append((what, rel_l2(got, g[k])))
    return out


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_backward_block_by_block_vs_twin(name):
    r = run(name)
    errs = block_errors(r)
    worst = {f: max(v, key=lambda e: e[1]) for f, v in errs.items()}
    print("\nnet %s, HIP vs twin, worst rel-L2 per family: %s" % (name, ", ".join("%s %.3e (%s)" % (f, w[1], w[0]) for f, w in worst.items())))
    for f, bound in (("dx_in", BOUND_DX), ("ln", BOUND_LN), ("weight", BOUND_W), ("bias", BOUND_B)):
        bad = [e for e in errs[f] if not e[1] < bound]
        assert not bad, (f, bound, bad)


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_token_tail(name):
    """pos_embed and cls_token: fp32 sums over the samples, in ascending order, of stored bf16 values -> bit for bit; the patch rows a plain copy;
    the patch embedding's weight and bias gradient (the weight-gradient launch without a data gradient) against fp64 of the plan's own dpe"""
    r = run(name)
    P = r.P
    B, T, C = P.B, P.T, P.C
    d0 = r.d_in[-1].reshape(B, T, C)
    assert same_bits(r.grad_cur_after_tail.reshape(B, T, C), d0)                 # the tail does not touch the token gradient
    assert same_bits(r.dpe, d0[:, 1:].contiguous())
    g = TW.backward_tokens(d0.float().reshape(B * T, C), r.t["patches"].float(), B, 16)
    assert same_bits(P.grad(r.flat, "base.pos_embed"), g["base.pos_embed"]), "pos_embed gradient"
    assert same_bits(P.grad(r.flat, "base.cls_token"), g["base.cls_token"]), "cls_token gradient"
    # dW = dpe^T patches, db = column sums of dpe over R = B (T - 1) rows in fp32, split and summed in a fixed but unspecified order: every
    # partial sum is bounded by the sum of magnitudes, at most R + 2 roundings of 2^-23
    dpe, pt = r.dpe.reshape(-1, C).double(), r.t["patches"].double()
    R = dpe.shape[0]
    assert_within(P.grad(r.flat, "base.patch_embed.proj.weight").reshape(C, -1).double(), dpe.t() @ pt, (R + 2) * U1 * (dpe.abs().t() @ pt.abs()), "patch weight gradient")
    assert_within(P.grad(r.flat, "base.patch_embed.proj.bias").double(), dpe.sum(0), (R + 2) * U1 * dpe.abs().sum(0), "patch bias gradient")


# ---------------------------------------------------------------------------------------------------------------------------------------
# (d) stages and determinism
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["D", "B"])
def test_stages_debug_calls_and_whole_backward_agree_bit_for_bit(name):
    r = run(name)
    P, net = r.P, r.net
    _lib, L = _dbg()
    plan = net._last_plan
    dg = r.d_feat.cuda()
    n_st = plan.n_stages
    ranges = [plan.stage_range(s) for s in range(n_st)]
    # the ranges tile [0, param_elems) without overlap, later stages below earlier ones
    assert ranges[0][1] == plan.param_elems and ranges[-1][0] == 0
    for s in range(n_st):
        assert ranges[s][0] < ranges[s][1]
        if s:
            assert ranges[s][1] == ranges[s - 1][0]
    if name == "D":
        sizes = [sum(1 for i in range(P.depth) if b <= P.table["base.blocks.%d.norm1.weight" % i][0] < e) for b, e in ranges]
        assert sizes == [1, 2, 1, 2], sizes
    # (1) the whole backward
    nan_fill(net)
    _lib.check(L.dali_vit_backward(plan.h, _lib.stream_ptr(), _lib.ptr(dg)), "dali_vit_backward")
    whole = net.flat_grads.cpu()
    # (2) stage by stage: after stages 0 .. s the slice of stage s already holds its final bits (the data-parallel reducer sends it then)
    nan_fill(net)
    for s in range(n_st):
        _lib.check(L.dali_vit_backward_stages(plan.h, _lib.stream_ptr(), _lib.ptr(dg), s, s), "dali_vit_backward_stages")
        now = net.flat_grads.cpu()
        for s2 in range(s + 1):
            b, e = ranges[s2]
            assert same_bits(now[b:e], whole[b:e]), "after stage %d the range of stage %d is not final" % (s, s2)
        for s2 in range(s + 1, n_st):
            b, e = ranges[s2]
            assert bool((bits(now[b:e]) == SENTINEL).all()), "stage %d wrote into the range of stage %d" % (s, s2)
    assert same_bits(now, whole)
    # (3) the block-by-block debug calls (run() made them right after the forward)
    assert same_bits(r.flat, whole)
