"""The ResNet plan's WIRING (daliid_amd/csrc/resnet_plan.hip), op by op, from the plan's own tensors.

Every kernel the plan launches is held tightly on its own (tests/test_gpu_conv_plan_shapes.py, test_gpu_nnops_plan_sizes.py, test_gpu_bnlin.py,
test_gpu_plan_only.py); how block_forward / block_backward string them together was checked only one whole bottleneck at a time against the
rounding-matched twin (tests/test_gpu_resnet_blocks.py: 6e-3 on an output, 4e-2 on a gradient), inside which a weight-gradient sum short of a
pixel row, a neighbour's BatchNorm coefficients or a missing mask fit (tests/test_resnet_twin_cpu.py measures by how much).  Here:

 (a) forward: every stored tensor against its op applied in fp64 to the plan's own stored inputs and bf16 weight images;
 (b) backward: every intermediate (kept by dali_debug_resnet_backward_block_snap, which copies each one right after the launch that produces it:
     the backward reuses its buffers in place) and every gradient slot against fp64 from the plan's own stored operands and the plan's own
     incoming gradient, so that errors do not chain;
 (c) dali_resnet_backward == the stages one by one == the per-block debug calls == the snapshot-mode calls, bit for bit; every parameter slot is
     written; a stage's parameter range is final once the stage has run.

Three kinds of bound (tests/resnet_checks.py):
  exact    a1 / a2 from the plan's own scale / shift, the recomputed ReLU mask, ybits, pool0 / pool_arg, head_arg, the merged image's (A.W)^T half,
           dbeta of the moments scheme (= colsum(dz)), zeros under a mask, the stem gradient's unpack, everything of (c);
  derived  convolution, GEMM, column-sum and BatchNorm-sum outputs: one bf16 store (half an ulp) plus the fp32 accumulation bound over the number of
           terms on the sum of magnitudes (sum_bound), written next to each assertion;
  twin     cancellation-prone quantities (invstd and what hangs on it; dgamma / dW finished through the moments): the HIP value may be at most 2 x
           as far from fp64 as the rounding-matched twin's same op (oracle/resnet50_bf16.py: _conv, _bn_train, _Conv3Bn3Moments) on the same inputs,
           plus the derived floor of the quantity's straightforward form.  Both figures are printed; docs/experiments.md, "ResNet plan, op by op".

Nets (Encoders.ResNet50ReID in train mode, random weights, non-trivial BatchNorm affines and running statistics):
  R1  width 32, layers (1, 2, 1, 2), batch 8 of 64 x 32: 1024 / 256 / 64 / 64 pixels (the last two below one GEMM tile)
  R2  width 64, layers (1, 1, 1, 1), batch 6 of 96 x 48: 1728 / 432 / 108 / 108 pixels (ragged against every tile; 3-wide maps in layer3 / 4)
"""
import ctypes
import functools
import time
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import resnet50_bf16 as M
from oracle.resnet50_reid import ResNet50ReID as OracleNet
from resnet_checks import HB, U, _bn1d_check_y, _pack_bits, check_bn_bwd_general, check_stored, check_twin_relative, sum_bound, ulp32
from vit_checks import assert_within as _assert_within, check_bn1d_bwd          # (NaN counts as off)

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
f32 = torch.float32
EPS = float(np.float32(1e-5))
MOM = float(np.float32(0.1))
SENTINEL = 0x7FC0BEEF               # a quiet NaN with a recognisable payload, as int32
DALI_ERR_INVALID = -1               # include/daliid.h
# include/daliid_debug.h
(SNAP_D_A2, SNAP_D_RAW2, SNAP_D_A1, SNAP_D_RAW1, SNAP_D_RAWD, SNAP_DX_CONV1, SNAP_G0_CONV3, SNAP_G0_DS, SNAP_D_RAW0, SNAP_STEM_DW_PAD, SNAP_HEAD_DZ,
 SNAP_COUNT) = range(12)
SNAP_BYTES = 32 << 20

NETS = {"R1": dict(width=32, layers=(1, 2, 1, 2), N=8, H=64, W=32),
        "R2": dict(width=64, layers=(1, 1, 1, 1), N=6, H=96, W=48)}


def bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == bf16 else torch.int32)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def _dbg():
    """the diagnostic entry points (include/daliid_debug.h), bound here: nothing under daliid_amd/ binds them"""
    from daliid_amd import _lib
    L = _lib.lib()
    vp = ctypes.c_void_p
    L.dali_debug_resnet_backward_block.argtypes = [vp, vp, vp, ctypes.c_int]
    L.dali_debug_resnet_backward_block_snap.argtypes = [vp, vp, vp, ctypes.c_int, vp, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    return _lib, L


def geometry(cfg):
    """per block: dict(li, hin, win, hout, wout, cin, w, cout, stride, has_ds, lin_ds, name)"""
    h, w, inpl, out = cfg["H"] // 4, cfg["W"] // 4, cfg["width"], []
    for li, nb in enumerate(cfg["layers"]):
        planes = cfg["width"] << li
        for bi in range(nb):
            st = (1, 2, 2, 1)[li] if bi == 0 else 1
            g = dict(li=li, hin=h, win=w, hout=h // st, wout=w // st, cin=inpl, w=planes, cout=4 * planes, stride=st, has_ds=bi == 0,
                     lin_ds=not out, name="layer%d.%d" % (li + 1, bi))
            h, w, inpl = g["hout"], g["wout"], 4 * planes
            out.append(g)
    return out


def make_net(cfg, seed=4):
    """as tests/test_gpu_resnet_blocks.py: random weights, BatchNorm affines 0.5 + U(0, 1) / 0.2 N(0, 1); here the running statistics are
    non-trivial too (the eval walk and the momentum update then see a wrong operand)"""
    from daliid_amd import Encoders
    torch.manual_seed(seed)
    ref = OracleNet(layers=cfg["layers"], width=cfg["width"])
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm1d)):
                m.weight.copy_(0.5 + torch.rand(m.weight.shape, generator=g))
                m.bias.copy_(0.2 * torch.randn(m.bias.shape, generator=g))
                m.running_mean.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.bias.shape, generator=g))
    net = Encoders.ResNet50ReID(layers=cfg["layers"], width=cfg["width"])
    net.load_state_dict(ref.state_dict())
    return net, ref, g


class Plan:
    def __init__(self, net, cfg):
        self.net, self.cfg, self.geo = net, cfg, geometry(cfg)
        self.N = cfg["N"]
        plan = net._plan(cfg["N"], cfg["H"], cfg["W"])
        self.ptable = {name: (off, numel, shape) for name, off, numel, shape in plan.tensor_table(0)}
        self.btable = {name: (off, numel, shape) for name, off, numel, shape in plan.tensor_table(1)}

    def get(self, name, dtype, *shape):
        return self.net.debug_tensor(name, dtype, shape).cpu()

    def status(self, name):
        _lib, L = _dbg()
        ptr, nbytes = ctypes.c_void_p(), ctypes.c_int64()
        return L.dali_resnet_debug_tensor(self.net._last_plan.h, name.encode(), ctypes.byref(ptr), ctypes.byref(nbytes))

    @staticmethod
    def seg(flat, entry):
        """a table entry of a flat host buffer in its STORED order (a conv weight: [cout][r][s][cin])"""
        off, numel, shape = entry
        v = flat[off:off + numel]
        if len(shape) == 4:
            o, i, r, s = shape
            return v.view(o, r, s, i)
        return v.view(*shape)

    def param(self, flat, name):
        return self.seg(flat, self.ptable[name])

    def buf(self, flat, name):
        return self.seg(flat, self.btable[name])


def read_bn(P, prefix):
    out = {}
    for k in ("scale", "shift", "mean", "invstd"):
        out[k] = P.get(prefix + "." + k, f32, -1)
    return out


def forward_tensors(P, training=True):
    N, cfg = P.N, P.cfg
    wb = cfg["width"]
    sh, sw, ph, pw = cfg["H"] // 2, cfg["W"] // 2, cfg["H"] // 4, cfg["W"] // 4
    t = {"pool0": P.get("pool0", bf16, N, ph, pw, wb), "w_stem": P.get("w_stem", bf16, wb, 7, 8, 4), "bn1": read_bn(P, "bn1"),
         "feat": P.get("feat", f32, N, -1), "head_arg": P.get("head_arg", torch.int16, N, -1),
         "neck.mean": P.get("neck.mean", f32, -1), "neck.invstd": P.get("neck.invstd", f32, -1)}
    if training:
        t["raw0"] = P.get("raw0", bf16, N, sh, sw, wb)
        t["pool_arg"] = P.get("pool_arg", torch.uint8, N, ph, pw, wb)
    for i, g in enumerate(P.geo):
        b = "block%d." % i
        t[b + "a1"] = P.get(b + "a1", bf16, N, g["hin"], g["win"], g["w"])
        t[b + "a2"] = P.get(b + "a2", bf16, N, g["hout"], g["wout"], g["w"])
        t[b + "y"] = P.get(b + "y", bf16, N, g["hout"], g["wout"], g["cout"])
        convs = (("1", g["w"], 1, g["cin"]), ("2", g["w"], 3, g["w"]), ("3", g["cout"], 1, g["w"])) + ((("d", g["cout"], 1, g["cin"]),) if g["has_ds"] else ())
        for c, co, k, ci in convs:
            t[b + "conv%s.w" % c] = P.get(b + "conv%s.w" % c, bf16, co, k, k, ci)
            t[b + "bn" + c] = read_bn(P, b + "bn" + c)
        if g["has_ds"]:
            t[b + "rawd"] = P.get(b + "rawd", bf16, N, g["hout"], g["wout"], g["cout"])
        if training:
            t[b + "raw1"] = P.get(b + "raw1", bf16, N, g["hin"], g["win"], g["w"])
            t[b + "raw2"] = P.get(b + "raw2", bf16, N, g["hout"], g["wout"], g["w"])
            t[b + "ybits"] = P.get(b + "ybits", torch.uint8, -1)
            for l, w_, C_ in (("l3", g["w"], g["cout"]),) + ((("ld", g["cin"], g["cout"]),) if g["lin_ds"] else ()):
                t[b + l + ".gram"] = P.get(b + l + ".gram", f32, w_, w_)
                t[b + l + ".m2"] = P.get(b + l + ".m2", f32, w_)
                t[b + l + ".ut"] = P.get(b + l + ".ut", f32, w_, C_)
    return t


@functools.lru_cache(maxsize=None)
def run(name):
    """one training forward and one snapshot-mode block-by-block backward of net `name`; everything the tests of (a) and (b) read, on the host"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    t0 = time.time()
    torch.set_num_threads(min(16, max(torch.get_num_threads(), 8)))
    cfg = NETS[name]
    net, ref, g = make_net(cfg)
    net.train(); ref.train()
    P = Plan(net, cfg)
    _lib, L = _dbg()
    x = torch.randn(cfg["N"], 3, cfg["H"], cfg["W"], generator=g)
    d_emb = torch.randn(cfg["N"], cfg["width"] * 32, generator=g)
    r = types.SimpleNamespace(P=P, net=net, ref=ref, cfg=cfg, x=x, d_emb=d_emb, geo=P.geo)
    r.buffers0 = net.flat_buffers.cpu().clone()
    r.emb = net._run_forward(x.cuda(), True).cpu()
    r.buffers1 = net.flat_buffers.cpu().clone()
    r.params = net.flat_params.detach().cpu().clone()
    r.t = forward_tensors(P)
    # backward, one block at a time, keeping the in-place intermediates
    bits(net.flat_grads).fill_(SENTINEL)
    snap = torch.zeros(SNAP_BYTES, dtype=torch.uint8, device="cuda")
    offs = (ctypes.c_int64 * SNAP_COUNT)()
    dg = d_emb.cuda()
    plan = net._last_plan.h
    r.snaps, r.dz_in, r.dx_out = {}, {}, {}
    nb = len(P.geo)

    def call(block):
        _lib.check(L.dali_debug_resnet_backward_block_snap(plan, _lib.stream_ptr(), _lib.ptr(dg), block, _lib.ptr(snap), SNAP_BYTES, offs),
                   "dali_debug_resnet_backward_block_snap")
        torch.cuda.synchronize()
        host = snap.cpu()
        return [int(o) for o in offs], host

    def cut(host, off, dtype, *shape):
        n = int(np.prod(shape)) * (2 if dtype == bf16 else 4)
        assert off >= 0 and off % 256 == 0 and off + n <= SNAP_BYTES
        return host[off:off + n].clone().view(dtype).view(*shape)

    for bi in range(nb - 1, -1, -1):
        gm = P.geo[bi]
        N = P.N
        if bi < nb - 1:
            r.dz_in[bi] = P.get("grad_cur", bf16, N, gm["hout"], gm["wout"], gm["cout"])
        o, host = call(bi)
        s = {"d_a2": cut(host, o[SNAP_D_A2], bf16, N, gm["hout"], gm["wout"], gm["w"]), "d_raw2": cut(host, o[SNAP_D_RAW2], bf16, N, gm["hout"], gm["wout"], gm["w"]),
             "d_a1": cut(host, o[SNAP_D_A1], bf16, N, gm["hin"], gm["win"], gm["w"]), "d_raw1": cut(host, o[SNAP_D_RAW1], bf16, N, gm["hin"], gm["win"], gm["w"]),
             "G0": cut(host, o[SNAP_G0_CONV3], f32, gm["cout"], gm["w"])}
        assert (o[SNAP_D_RAWD] >= 0) == (gm["has_ds"] and not gm["lin_ds"]) and (o[SNAP_DX_CONV1] >= 0) == gm["has_ds"]
        assert (o[SNAP_G0_DS] >= 0) == gm["lin_ds"] and (o[SNAP_HEAD_DZ] >= 0) == (bi == nb - 1) and o[SNAP_D_RAW0] < 0 and o[SNAP_STEM_DW_PAD] < 0
        if o[SNAP_D_RAWD] >= 0:
            s["d_rawd"] = cut(host, o[SNAP_D_RAWD], bf16, N, gm["hout"], gm["wout"], gm["cout"])
        if gm["has_ds"]:
            s["dx_conv1"] = cut(host, o[SNAP_DX_CONV1], bf16, N, gm["hin"], gm["win"], gm["cin"])
        if gm["lin_ds"]:
            s["G0d"] = cut(host, o[SNAP_G0_DS], f32, gm["cout"], gm["cin"])
        if bi == nb - 1:
            r.dz_in[bi] = cut(host, o[SNAP_HEAD_DZ], bf16, N, gm["hout"], gm["wout"], gm["cout"])
            r.dfeat = P.get("dfeat", f32, N, -1)
        assert same_bits(P.get("block%d.d_raw1" % bi, bf16, N, gm["hin"], gm["win"], gm["w"]), s["d_raw1"])       # the older name reads the same tensor
        b = "block%d." % bi
        s["sdz"] = P.get(b + "sdz", f32, -1)
        for l, w_ in (("l3", gm["w"]),) + ((("ld", gm["cin"]),) if gm["lin_ds"] else ()):
            s[l + ".wd"] = P.get(b + l + ".wd", bf16, w_, gm["cout"] + w_)
            s[l + ".bvec"] = P.get(b + l + ".bvec", f32, w_)
            s[l + ".qk"] = P.get(b + l + ".qk", f32, 2, gm["cout"])
        r.snaps[bi] = s
        r.dx_out[bi] = P.get("grad_cur", bf16, N, gm["hin"], gm["win"], gm["cin"])
    o, host = call(-1)
    wb = cfg["width"]
    r.d_raw0 = cut(host, o[SNAP_D_RAW0], bf16, P.N, cfg["H"] // 2, cfg["W"] // 2, wb)
    r.stem_dw_pad = cut(host, o[SNAP_STEM_DW_PAD], f32, wb, 7, 8, 4)
    assert same_bits(P.get("d_raw0", bf16, P.N, cfg["H"] // 2, cfg["W"] // 2, wb), r.d_raw0)
    r.flat = net.flat_grads.cpu().clone()
    r.report = []
    print("\nnet %s: forward + snapshot-mode backward + read-back %.1f s" % (name, time.time() - t0))
    return r


# ---------------------------------------------------------------------------------------------------------------------------------------
# fp64 operators on the plan's layouts (activations NHWC, weights [cout][r][s][cin]); each returns the value and the accumulation bound
# ---------------------------------------------------------------------------------------------------------------------------------------
def nchw(t):
    return t.permute(0, 3, 1, 2).double()


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def oihw(w):
    return w.permute(0, 3, 1, 2).double()


def conv64(x, w, stride, pad):
    """fp64 convolution and the fp32 accumulation bound over K = r s cin terms on sum |x| |w|"""
    xd, wd = nchw(x), oihw(w)
    K = wd[0].numel()
    return nhwc(F.conv2d(xd, wd, stride=stride, padding=pad)), sum_bound(K, nhwc(F.conv2d(xd.abs(), wd.abs(), stride=stride, padding=pad)))


def dgrad64(dy, w, stride, pad, hin, win):
    """fp64 data gradient of the convolution and its bound over at most K = r s cout terms"""
    dyd, wd = nchw(dy), oihw(w)
    size = (dyd.shape[0], wd.shape[1], hin, win)
    K = wd.shape[0] * wd.shape[2] * wd.shape[3]
    ref = torch.nn.grad.conv2d_input(size, wd, dyd, stride=stride, padding=pad)
    mag = torch.nn.grad.conv2d_input(size, wd.abs(), dyd.abs(), stride=stride, padding=pad)
    return nhwc(ref), sum_bound(K, nhwc(mag))


def wgrad64(x, dy, k, stride, pad):
    """fp64 weight gradient [cout][r][s][cin] and its bound: sums over the P output pixels (split-K slabs and their reduction included)"""
    xd, dyd = nchw(x), nchw(dy)
    shape = (dyd.shape[1], xd.shape[1], k, k)
    P = dyd.shape[0] * dyd.shape[2] * dyd.shape[3]
    ref = torch.nn.grad.conv2d_weight(xd, shape, dyd, stride=stride, padding=pad)
    mag = torch.nn.grad.conv2d_weight(xd.abs(), shape, dyd.abs(), stride=stride, padding=pad)
    return ref.permute(0, 2, 3, 1).contiguous(), sum_bound(P, mag.permute(0, 2, 3, 1).contiguous())


def inv_err(var, dvar):
    """how far 1 / sqrt(var + eps) moves when var moves by at most dvar (either way), + its fp32 rounding"""
    inv = 1.0 / torch.sqrt(var + EPS)
    lo = 1.0 / torch.sqrt((var - dvar).clamp_min(0) + EPS)
    return (lo - inv) + ulp32(inv)


def twin_stats(u):
    """oracle.resnet50_bf16._bn_train's statistics of the fp32 convolution result u (NCHW): mean, invstd"""
    mean = u.mean((0, 2, 3))
    var = u.var((0, 2, 3), unbiased=False)
    return mean, 1.0 / torch.sqrt(var + 1e-5)


def check_bn_stats(r, bn, u, E, x_twin, conv_mod, gamma, beta, rm, rv, what, moments=None):
    """A training-mode BatchNorm's stored mean / invstd / scale / shift and running statistics against the fp64 statistics of the fp64
    convolution u [N, H, W, C] (accumulators within E of it).  mean: derived.  invstd, scale, shift: cancellation-prone (E[x^2] - mean^2),
    twin-relative with the derived floor.  moments: (dmean, dvar) of the moments scheme, else the floor of the tile-sum scheme:
      mean: every accumulator within E, the fp32 tile sums and their fp64 finish over P terms, one rounding;
      E[x^2]: 2|u|E + E^2 per term, the same sums;  var = E[x^2] - mean^2: + 2|mean| dmean + dmean^2."""
    C = u.shape[-1]
    u2 = u.reshape(-1, C)
    Pn = u2.shape[0]
    mean64, var64 = u2.mean(0), u2.var(0, unbiased=False)
    inv64 = 1.0 / torch.sqrt(var64 + EPS)
    if moments is None:
        E2 = E.reshape(-1, C)
        dmean = E2.mean(0) + sum_bound(Pn, u2.abs().sum(0)) / Pn + ulp32(mean64)
        dvar = (2 * u2.abs() * E2 + E2 * E2).mean(0) + sum_bound(Pn, (u2 * u2).sum(0)) / Pn + 2 * mean64.abs() * dmean + dmean * dmean
    else:
        dmean, dvar = moments
    _assert_within(bn["mean"].double(), mean64, dmean, what + " mean")
    dinv = inv_err(var64, dvar)
    with torch.no_grad():
        tm, ti = twin_stats(M._conv(x_twin, conv_mod))
    g64, b64 = gamma.double(), beta.double()
    sc64 = g64 * inv64
    dsc = g64.abs() * dinv + ulp32(sc64)
    sh64 = b64 - mean64 * sc64
    dsh = mean64.abs() * dsc + sc64.abs() * dmean + 2 * U * (b64.abs() + (mean64 * sc64).abs())
    tsc = gamma * ti
    for k, got, tw, ref, d in (("invstd", bn["invstd"], ti, inv64, dinv), ("scale", bn["scale"], tsc, sc64, dsc), ("shift", bn["shift"], beta - tm * tsc, sh64, dsh)):
        check_twin_relative(got, tw, ref, float(d.norm() / ref.norm()), what + " " + k, r.report)
    # the stored coefficients hang together exactly as the finishing kernels form them: scale = fp32(gamma * invstd), shift = fp32(beta - fp32(mean) * scale)
    assert same_bits(bn["scale"], gamma * bn["invstd"]), what + ": scale is not gamma * invstd"
    assert same_bits(bn["shift"], beta - bn["mean"] * bn["scale"]), what + ": shift is not beta - mean * scale"
    # running statistics: (1 - m) r + m s with m = 0.1f, s = the batch mean / the UNBIASED variance; from the plan's own mean and invstd
    # (var = 1 / invstd^2 - eps, within 4u (var + eps) of what the kernel held): the fp32 constants, two products, one sum <= 6u of the magnitudes
    m0, m1 = r.P.buf(r.buffers0, rm).double(), r.P.buf(r.buffers1, rm).double()
    v0, v1 = r.P.buf(r.buffers0, rv).double(), r.P.buf(r.buffers1, rv).double()
    mk, ik = bn["mean"].double(), bn["invstd"].double()
    vk = (1.0 / (ik * ik) - EPS)
    unb = vk * Pn / (Pn - 1.0)
    _assert_within(m1, (1 - MOM) * m0 + MOM * mk, 6 * U * ((0.9 * m0).abs() + (0.1 * mk).abs()), what + " running_mean")
    _assert_within(v1, (1 - MOM) * v0 + MOM * unb, 6 * U * ((0.9 * v0).abs() + (0.1 * unb).abs()) + MOM * 4 * U * (vk + EPS) * Pn / (Pn - 1.0), what + " running_var")


def act_exact(raw, bn):
    """dali_bn_act as test_bn_act_plan_sizes emulates it: fp32 raw * scale + shift (product, then sum: no contraction), ReLU, one bf16 rounding"""
    z = raw.float() * bn["scale"] + bn["shift"]
    return z.clamp(min=0).to(bf16), z > 0


def twin_in(x):
    """a stored NHWC bf16 tensor as the twin's fp32 NCHW operand"""
    return x.float().permute(0, 3, 1, 2).contiguous()


# ---------------------------------------------------------------------------------------------------------------------------------------
# (a) forward
# ---------------------------------------------------------------------------------------------------------------------------------------
def ref_blocks(ref):
    return [b for l in (ref.layer1, ref.layer2, ref.layer3, ref.layer4) for b in l]


@pytest.mark.parametrize("name", ["R1", "R2"])
def test_forward_op_by_op(name):
    r = run(name)
    P, t, cfg = r.P, r.t, r.cfg
    N, wb = P.N, cfg["width"]
    prm = lambda k: P.param(r.params, k)
    # ---- weight images: the bf16 cast of the master weights, in the stored order ----
    stem_w = prm("conv1.weight")                                                 # [wb][7][7][3]
    pad = torch.zeros(wb, 7, 8, 4)
    pad[:, :, :7, :3] = stem_w
    assert same_bits(t["w_stem"], pad.to(bf16)), "w_stem"
    # ---- stem: raw0 = conv7x7/2 of the bf16 image, bn1 (no ReLU), 3x3/2 max-pool with its tap ----
    ximg = r.x.permute(0, 2, 3, 1).contiguous().to(bf16)                         # the packed image holds the bf16 cast (tests/test_gpu_plan_only.py)
    u, E = conv64(ximg, stem_w.to(bf16), 2, 3)
    check_stored(t["raw0"], u, E, "raw0")
    check_bn_stats(r, t["bn1"], u, E, twin_in(ximg), r.ref.conv1, prm("bn1.weight"), prm("bn1.bias"), "bn1.running_mean", "bn1.running_var", "stem bn1")
    z = (t["raw0"].float() * t["bn1"]["scale"] + t["bn1"]["shift"]).permute(0, 3, 1, 2)
    ph, pw = cfg["H"] // 4, cfg["W"] // 4
    cols = F.unfold(F.pad(z, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(N, wb, 9, ph * pw)
    a = cols.argmax(2)
    m = cols.gather(2, a.unsqueeze(2)).squeeze(2)
    to_nhwc = lambda v: v.view(N, wb, ph, pw).permute(0, 2, 3, 1)
    assert same_bits(t["pool0"], to_nhwc(m).to(bf16).contiguous()), "pool0"
    first = (cols == m.unsqueeze(2)).float().argmax(2)                           # first maximum in (r, s) scan order
    assert torch.equal(t["pool_arg"], to_nhwc(first).to(torch.uint8).contiguous()), "pool_arg"
    # ---- blocks ----
    x = t["pool0"]
    blocks = ref_blocks(r.ref)
    for i, g in enumerate(P.geo):
        b, pre, what, blk = "block%d." % i, g["name"] + ".", "net %s %s " % (name, g["name"]), blocks[i]
        W = lambda c: t[b + "conv%s.w" % c]
        for c, long_ in (("1", "conv1"), ("2", "conv2"), ("3", "conv3")) + ((("d", "downsample.0"),) if g["has_ds"] else ()):
            assert same_bits(W(c), prm(pre + long_ + ".weight").to(bf16)), what + "weight image " + c
        bnp = lambda c, k: prm(pre + ("downsample.1" if c == "d" else "bn" + c) + "." + k)
        bnb = lambda c, k: pre + ("downsample.1" if c == "d" else "bn" + c) + "." + k
        # conv1 -> raw1 (one bf16 store of K = cin products), bn1 from its accumulators, a1 bit for bit
        u, E = conv64(x, W("1"), 1, 0)
        check_stored(t[b + "raw1"], u, E, what + "raw1")
        check_bn_stats(r, t[b + "bn1"], u, E, twin_in(x), blk.conv1, bnp("1", "weight"), bnp("1", "bias"), bnb("1", "running_mean"), bnb("1", "running_var"), what + "bn1")
        a1, _ = act_exact(t[b + "raw1"], t[b + "bn1"])
        assert same_bits(t[b + "a1"], a1), what + "a1"
        # conv2 (3x3, the block's stride; K = 9 w) -> raw2, bn2, a2; the mask the backward recomputes from raw2 is the mask of a2
        u, E = conv64(t[b + "a1"], W("2"), g["stride"], 1)
        check_stored(t[b + "raw2"], u, E, what + "raw2")
        check_bn_stats(r, t[b + "bn2"], u, E, twin_in(t[b + "a1"]), blk.conv2, bnp("2", "weight"), bnp("2", "bias"), bnb("2", "running_mean"), bnb("2", "running_var"), what + "bn2")
        a2, mask2 = act_exact(t[b + "raw2"], t[b + "bn2"])
        assert same_bits(t[b + "a2"], a2), what + "a2"
        assert torch.equal(mask2, t[b + "a2"].float() > 0), what + "recomputed ReLU mask != (a2 > 0)"
        # the moments of a2 (a2 >= 0: magnitudes = values): gram and m2 are sums over the P pixels; ut = (W3 G)^T, w terms, from the plan's own gram
        a2d = t[b + "a2"].double().reshape(-1, g["w"])
        Pn = a2d.shape[0]
        G64, m264 = a2d.t() @ a2d, a2d.sum(0)
        dG, dm2 = sum_bound(Pn, G64), sum_bound(Pn, m264)
        _assert_within(t[b + "l3.gram"].double(), G64, dG, what + "l3.gram")
        _assert_within(t[b + "l3.m2"].double(), m264, dm2, what + "l3.m2")
        w3 = W("3").double().reshape(g["cout"], g["w"])
        Gk = t[b + "l3.gram"].double()
        _assert_within(t[b + "l3.ut"].double(), Gk @ w3.t(), sum_bound(g["w"], Gk.abs() @ w3.abs().t()), what + "l3.ut")
        # bn3's statistics from the moments against the fp64 statistics of fp64 conv3(a2):  mean = W3 m2 / P (fp64 from the fp32 m2),
        # E[u^2] = rowdot(W3, W3 G) / P: G within dG, the product's w terms, the per-tile fp32 partial sums of the row dot (w terms)
        u3, E3 = conv64(t[b + "a2"], W("3"), 1, 0)
        w3a = w3.abs()
        dmean = (w3a @ dm2) / Pn + ulp32(u3.reshape(-1, g["cout"]).mean(0))
        dq = ((w3a @ dG) * w3a).sum(1) + 2 * sum_bound(g["w"], ((w3a @ G64) * w3a).sum(1))
        mean3 = u3.reshape(-1, g["cout"]).mean(0)
        dvar = dq / Pn + 2 * mean3.abs() * dmean + dmean * dmean
        check_bn_stats(r, t[b + "bn3"], u3, E3, twin_in(t[b + "a2"]), blk.conv3, bnp("3", "weight"), bnp("3", "bias"), bnb("3", "running_mean"), bnb("3", "running_var"),
                       what + "bn3 (moments)", moments=(dmean, dvar))
        # y = relu(scale3 acc + shift3 + identity) from the plan's own coefficients; identity = x, or rawd scale_d + shift_d
        s3, h3 = t[b + "bn3"]["scale"].double(), t[b + "bn3"]["shift"].double()
        if g["has_ds"]:
            ud, Ed = conv64(x, W("d"), g["stride"], 0)
            check_stored(t[b + "rawd"], ud, Ed, what + "rawd")
            check_bn_stats(r, t[b + "bnd"], ud, Ed, twin_in(x), blk.downsample[0], bnp("d", "weight"), bnp("d", "bias"), bnb("d", "running_mean"), bnb("d", "running_var"), what + "bnd")
            sd, hd = t[b + "bnd"]["scale"].double(), t[b + "bnd"]["shift"].double()
            idn, idn_mag = t[b + "rawd"].double() * sd + hd, (t[b + "rawd"].double() * sd).abs() + hd.abs()
        else:
            idn = idn_mag = x.double()
            idn_mag = idn_mag.abs()
        zref = s3 * u3 + h3 + idn
        # the output stage's fp32 terms: two products, three sums, each rounding <= u of the magnitudes so far: 6u of their total
        Ez = s3.abs() * E3 + 6 * U * ((s3 * u3).abs() + h3.abs() + idn_mag)
        check_stored(t[b + "y"], zref.clamp(min=0), Ez, what + "y")
        assert torch.equal(t[b + "ybits"], _pack_bits(t[b + "y"].float() > 0)), what + "ybits are not the bits of y > 0"
        if g["lin_ds"]:
            xd = x.double().reshape(-1, g["cin"])
            _assert_within(t[b + "ld.gram"].double(), xd.t() @ xd, sum_bound(Pn, xd.abs().t() @ xd.abs()), what + "ld.gram")
            _assert_within(t[b + "ld.m2"].double(), xd.sum(0), sum_bound(Pn, xd.abs().sum(0)), what + "ld.m2")
            wdd, Gk = W("d").double().reshape(g["cout"], g["cin"]), t[b + "ld.gram"].double()
            _assert_within(t[b + "ld.ut"].double(), Gk @ wdd.t(), sum_bound(g["cin"], Gk.abs() @ wdd.abs().t()), what + "ld.ut")
        x = t[b + "y"]
    # ---- head: feat = mean + max over the map (fp32 sum of HW values >= 0, one quotient, one sum), first arg-max; the neck in training mode ----
    yl = x.double().reshape(N, -1, x.shape[-1])
    HW = yl.shape[1]
    fref = yl.mean(1) + yl.max(1).values
    _assert_within(t["feat"].double(), fref, sum_bound(HW, yl.sum(1)) / HW + 2 * U * fref.abs(), "feat")
    assert torch.equal(t["head_arg"], yl.argmax(1).to(torch.int16)), "head_arg"
    fd = t["feat"].double()
    m64 = fd.mean(0)
    i64 = 1.0 / torch.sqrt(((fd - m64) ** 2).sum(0) / N + EPS)
    _assert_within(t["neck.mean"].double(), m64, ulp32(m64), "neck mean")                     # as test_bn1d_train_plan_sizes
    _assert_within(t["neck.invstd"].double(), i64, ulp32(i64), "neck invstd")
    _bn1d_check_y(r.emb, t["feat"], m64, i64, prm("last_bn.weight"), prm("last_bn.bias"), "neck output")
    for k, s64 in (("last_bn.running_mean", m64), ("last_bn.running_var", ((fd - m64) ** 2).sum(0) / (N - 1))):                # momentum 0.1, unbiased
        r0, r1 = P.buf(r.buffers0, k).double(), P.buf(r.buffers1, k).double()
        _assert_within(r1, (1 - MOM) * r0 + MOM * s64, 6 * U * ((0.9 * r0).abs() + (0.1 * s64).abs()), k)
    print_report(r, "forward")


def print_report(r, stage):
    fam = {}
    key = lambda what: ("moments " if "moments" in what or " ld " in what or " l3 " in what else "") + what.split()[-1]
    for what, e_hip, e_twin, floor in r.report:
        k = key(what)
        cur = fam.get(k)
        if cur is None or e_hip - (2 * e_twin + floor) > cur[1] - (2 * cur[2] + cur[3]):
            fam[k] = (what, e_hip, e_twin, floor)
    print("\n%s, twin-relative quantities (rel-L2 against fp64), the one nearest its bound per family:" % stage)
    for k, (what, e_hip, e_twin, floor) in sorted(fam.items()):
        print("  %-28s HIP %.3e  twin %.3e  floor %.3e  bound %.3e   (%s)" % (k, e_hip, e_twin, floor, 2 * e_twin + floor, what))
    worst = {}
    for what, e_hip, e_twin, floor in r.report:
        w = worst.setdefault(key(what), [0.0, 0.0])
        w[0], w[1] = max(w[0], e_hip), max(w[1], e_twin)
    print("  maxima per family: " + ", ".join("%s HIP %.2e twin %.2e" % (k, v[0], v[1]) for k, v in sorted(worst.items())))
    del r.report[:]


def test_debug_tensor_names():
    r = run("R1")
    P = r.P
    for bad in ("nope", "block6.a2", "block-1.a2", "block0.nope", "block0.l3.nope", "block1.ld.gram", "block2.rawd", "block0.l3", "neck.nope"):
        assert P.status(bad) == DALI_ERR_INVALID, bad
    for good in ("block0.a2", "block5.ybits", "block0.sdz", "block0.ld.gram", "block0.ld.qk", "block3.l3.wd", "block1.l3.bvec", "pool_arg", "head_arg", "neck.mean",
                 "neck.invstd", "dfeat", "grad_cur", "d_raw0"):
        assert P.status(good) == 0, good


# ---------------------------------------------------------------------------------------------------------------------------------------
# (b) backward
# ---------------------------------------------------------------------------------------------------------------------------------------
def check_linbn_bwd(r, what, l, s, G0, sdz, dz2, xin2, w, bn, gamma, got_dW, got_dg, got_db, twin, has_bvec_ref=True):
    """The moments scheme's backward of bn(x W^T) (launch_bnlin_bwd) for one 1x1 convolution: dz2 [P][C], xin2 [P][w] (float64), w [C][w] bf16.
    twin: (dW, dgamma) of the rounding-matched twin's same op."""
    P_, C, wd_ = dz2.shape[0], dz2.shape[1], xin2.shape[1]
    # s = colsum(dz) and G0 = dz^T x: fp32 sums over the P pixels (derived)
    _assert_within(sdz.double(), dz2.sum(0), sum_bound(P_, dz2.abs().sum(0)), what + "sdz")
    _assert_within(G0.double(), dz2.t() @ xin2, sum_bound(P_, dz2.abs().t() @ xin2.abs()), what + "G0")
    assert same_bits(got_db, sdz), what + "dbeta is not colsum(dz)"                                   # (float)(double)s
    # fp64 reference of the op itself, from the fp64 convolution's own statistics
    w64 = w.double()
    u = xin2 @ w64.t()
    mean, var = u.mean(0), u.var(0, unbiased=False)
    inv = 1.0 / torch.sqrt(var + EPS)
    xh = (u - mean) * inv
    S1, S2 = dz2.sum(0), (dz2 * xh).sum(0)
    sc = gamma.double() * inv
    d_raw = sc * (dz2 - S1 / P_ - xh * (S2 / P_))
    dW64 = d_raw.t() @ xin2
    # dgamma and the finished dW: cancellation-prone (rowdot(W, G0) - mean s; A G0 + Kc m2 - Q (W G)) -> twin-relative; floors: the straightforward
    # sums over P pixels
    tw_dW, tw_dg = twin
    check_twin_relative(got_dg, tw_dg, S2, float(sum_bound(P_, (dz2 * xh).abs().sum(0)).norm() / S2.norm()), what + "dgamma", r.report)
    check_twin_relative(got_dW, tw_dW, dW64, float(sum_bound(P_, d_raw.abs().t() @ xin2.abs()).norm() / dW64.norm()), what + "dW", r.report)
    # Q, Kc from the plan's OWN dgamma, colsum, scale, mean, invstd (fp64 in the kernel, rounded once; dgamma was rounded before we read it: 2u):
    a, mk, ik, dgk, sk = bn["scale"].double(), bn["mean"].double(), bn["invstd"].double(), got_dg.double(), sdz.double()
    Q = a * ik * dgk / P_
    Kc = Q * mk - a * sk / P_
    _assert_within(s[l + ".qk"][0].double(), Q, 3 * U * Q.abs(), what + "Q")
    _assert_within(s[l + ".qk"][1].double(), Kc, 3 * U * ((Q * mk).abs() + (a * sk / P_).abs()), what + "Kc")
    # the merged data-gradient image [w][C + w]: (A.W)^T bit for bit (one fp32 product, one bf16 rounding); -(W^T diag(Q) W) a sum of C fp32 terms, one
    # bf16 store; bvec = W^T Kc, C terms -- from the plan's own Q and Kc
    wdimg = s[l + ".wd"]
    assert same_bits(wdimg[:, :C].contiguous(), (bn["scale"].unsqueeze(1) * w.float()).to(bf16).t().contiguous()), what + "wd (A.W)^T"
    Qk, Kk = s[l + ".qk"][0].double(), s[l + ".qk"][1].double()
    m2ref = -(w64.t() @ (Qk.unsqueeze(1) * w64))
    check_stored(wdimg[:, C:], m2ref, sum_bound(C, w64.abs().t() @ (Qk.abs().unsqueeze(1) * w64.abs())) + U * m2ref.abs(), what + "wd -(W^T diag(Q) W)")
    _assert_within(s[l + ".bvec"].double(), w64.t() @ Kk, sum_bound(C, w64.abs().t() @ Kk.abs()), what + "bvec")


@pytest.mark.parametrize("name", ["R1", "R2"])
def test_backward_op_by_op(name):
    r = run(name)
    P, t, cfg = r.P, r.t, r.cfg
    N = P.N
    prm = lambda k: P.param(r.params, k)
    grd = lambda k: P.param(r.flat, k)
    blocks = ref_blocks(r.ref)
    nb = len(P.geo)
    # ---- head: neck backward from the kernel's own statistics (check_bn1d_bwd), then the masked pooling gradient ----
    check_bn1d_bwd(r.dfeat, grd("last_bn.weight"), grd("last_bn.bias"), t["feat"], r.d_emb, prm("last_bn.weight"), t["neck.mean"].double(),
                   t["neck.invstd"].double(), "neck")
    gl = P.geo[-1]
    HW = gl["hout"] * gl["wout"]
    ylast = t["block%d.y" % (nb - 1)].reshape(N, HW, -1)
    d = r.dfeat.double().unsqueeze(1)
    hit = torch.arange(HW).view(1, HW, 1) == t["head_arg"].long().unsqueeze(1)
    ref = (d / HW + hit * d) * (ylast.float() > 0)
    got = r.dz_in[nb - 1].reshape(N, HW, -1)
    # (as _head_check_bwd: one bf16 rounding plus the fp32 rounding of the quotient and the sum)
    _assert_within(got.double(), ref, HB * ref.abs() + (1 + HB) * 2 * U * ((d / HW).abs() + ref.abs()), "head dz")
    assert bool((got.float()[ylast.float() <= 0] == 0).all()), "head dz is not 0 where y is 0"
    # ---- blocks, last first ----
    for i in range(nb - 1, -1, -1):
        g, s, b, blk = P.geo[i], r.snaps[i], "block%d." % i, blocks[i]
        pre, what = g["name"] + ".", "net %s %s " % (name, g["name"])
        W = lambda c: t[b + "conv%s.w" % c]
        x = t["pool0"] if i == 0 else t["block%d.y" % (i - 1)]
        dz = r.dz_in[i]
        Pout, Pin = N * g["hout"] * g["wout"], N * g["hin"] * g["win"]
        dz2, a22 = dz.double().reshape(Pout, -1), t[b + "a2"].double().reshape(Pout, -1)
        # -- bn3 + conv3 through the moments of a2: the twin's op on the same a2 / dz --
        a2t = twin_in(t[b + "a2"]).requires_grad_(True)
        w3p, g3p, b3p = (p_.detach().clone().requires_grad_(True) for p_ in (blk.conv3.weight, blk.bn3.weight, blk.bn3.bias))
        M._Conv3Bn3Moments.apply(a2t, w3p, g3p, b3p, 1e-5).backward(twin_in(dz))
        check_linbn_bwd(r, what + "l3 ", "l3", s, s["G0"], s["sdz"], dz2, a22, W("3").reshape(g["cout"], g["w"]), t[b + "bn3"], prm(pre + "bn3.weight"),
                        grd(pre + "conv3.weight").reshape(g["cout"], g["w"]), grd(pre + "bn3.weight"), grd(pre + "bn3.bias"),
                        (w3p.grad.reshape(g["cout"], g["w"]), g3p.grad))
        # -- d_a2 = [dz | a2] wd^T + bvec: ONE GEMM over K = cout + w from the plan's own merged image and bias (derived) --
        wd, bv = s["l3.wd"].double(), s["l3.bvec"].double()
        cat = torch.cat((dz2, a22), 1)
        ref = cat @ wd.t() + bv
        E = sum_bound(g["cout"] + g["w"], cat.abs() @ wd.abs().t() + bv.abs())
        check_stored(s["d_a2"].reshape(Pout, -1), ref, E, what + "d_a2")
        # -- bn2 + ReLU backward, in place, mask recomputed from raw2 --
        _, mask2 = act_exact(t[b + "raw2"], t[b + "bn2"])
        bn = {k: v.double() for k, v in t[b + "bn2"].items()}
        check_bn_bwd_general(s["d_raw2"].reshape(Pout, -1), grd(pre + "bn2.weight"), grd(pre + "bn2.bias"), (s["d_a2"].double() * mask2).reshape(Pout, -1),
                             t[b + "raw2"].double().reshape(Pout, -1), bn["mean"], bn["invstd"], bn["scale"], what + "bn2 backward")
        # -- conv2: weight gradient over the Pout pixels, data gradient over at most 9 w terms (stride 2: the parity split) --
        ref, E = wgrad64(t[b + "a1"], s["d_raw2"], 3, g["stride"], 1)
        _assert_within(grd(pre + "conv2.weight").double(), ref, E, what + "dW2")
        ref, E = dgrad64(s["d_raw2"], W("2"), g["stride"], 1, g["hin"], g["win"])
        check_stored(s["d_a1"], ref, E, what + "d_a1")
        # -- bn1 + ReLU backward --
        _, mask1 = act_exact(t[b + "raw1"], t[b + "bn1"])
        bn = {k: v.double() for k, v in t[b + "bn1"].items()}
        check_bn_bwd_general(s["d_raw1"].reshape(Pin, -1), grd(pre + "bn1.weight"), grd(pre + "bn1.bias"), (s["d_a1"].double() * mask1).reshape(Pin, -1),
                             t[b + "raw1"].double().reshape(Pin, -1), bn["mean"], bn["invstd"], bn["scale"], what + "bn1 backward")
        ref, E = wgrad64(x, s["d_raw1"], 1, 1, 0)
        _assert_within(grd(pre + "conv1.weight").double(), ref, E, what + "dW1")
        # -- dx: conv1's data gradient (+ the identity / the branch), masked with the previous block's ReLU bits (none for the net's first block) --
        prev_mask = (x.float() > 0) if i > 0 else torch.ones_like(x, dtype=torch.bool)
        c1, E1 = dgrad64(s["d_raw1"], W("1"), 1, 0, g["hin"], g["win"])
        dx = r.dx_out[i]
        if not g["has_ds"]:
            ref = (c1 + dz.double()) * prev_mask                                           # identity path: + dz
            check_stored(dx, ref, (E1 + U * (c1.abs() + dz.double().abs())) * prev_mask, what + "dx")
        else:
            check_stored(s["dx_conv1"], c1 * prev_mask, E1 * prev_mask, what + "dx after conv1's data gradient")
            base = s["dx_conv1"].double()
            if g["lin_ds"]:
                x2 = x.double().reshape(Pin, -1)
                xt = twin_in(x).requires_grad_(False)
                wdp, gdp, bdp = (p_.detach().clone().requires_grad_(True) for p_ in (blk.downsample[0].weight, blk.downsample[1].weight, blk.downsample[1].bias))
                ud = F.conv2d(xt, M.QW(wdp))
                M._bn_train(ud, M.QF(ud), types.SimpleNamespace(weight=gdp, bias=bdp)).backward(twin_in(dz))    # the stored rawd, its gradient never rounded (ds_through_moments)
                check_linbn_bwd(r, what + "ld ", "ld", s, s["G0d"], s["sdz"], dz2, x2, W("d").reshape(g["cout"], g["cin"]), t[b + "bnd"], prm(pre + "downsample.1.weight"),
                                grd(pre + "downsample.0.weight").reshape(g["cout"], g["cin"]), grd(pre + "downsample.1.weight"), grd(pre + "downsample.1.bias"),
                                (wdp.grad.reshape(g["cout"], g["cin"]), gdp.grad))
                wd, bv = s["ld.wd"].double(), s["ld.bvec"].double()
                cat = torch.cat((dz2, x2), 1)
                acc = cat @ wd.t() + bv
                ref = acc + base.reshape(Pin, -1)
                E = sum_bound(g["cout"] + g["cin"], cat.abs() @ wd.abs().t() + bv.abs()) + U * (acc.abs() + ref.abs())
                check_stored(dx.reshape(Pin, -1), ref, E, what + "dx (no mask on the net's first block)")
            else:
                bn = {k: v.double() for k, v in t[b + "bnd"].items()}
                check_bn_bwd_general(s["d_rawd"].reshape(Pout, -1), grd(pre + "downsample.1.weight"), grd(pre + "downsample.1.bias"), dz2,
                                     t[b + "rawd"].double().reshape(Pout, -1), bn["mean"], bn["invstd"], bn["scale"], what + "bnd backward")
                ref, E = wgrad64(x, s["d_rawd"], 1, g["stride"], 0)
                _assert_within(grd(pre + "downsample.0.weight").double(), ref, E, what + "dWd")
                cd, Ed = dgrad64(s["d_rawd"], W("d"), g["stride"], 0, g["hin"], g["win"])
                ref = (cd + base) * prev_mask
                check_stored(dx, ref, (Ed + U * (cd.abs() + base.abs())) * prev_mask, what + "dx")
                if g["stride"] == 2:                # only the even-even positions receive the branch: the other three parities keep conv1's bits
                    keep = torch.ones(g["hin"], g["win"], dtype=torch.bool)
                    keep[::2, ::2] = False
                    assert torch.equal(dx.float()[:, keep], s["dx_conv1"].float()[:, keep]), what + "dx off the even-even positions"
        if i > 0:
            assert bool((dx.float()[~prev_mask] == 0).all()), what + "dx is not 0 where the previous block's y is 0"
    # ---- stem: the max-pool's scatter through its taps, bn1 backward (no ReLU), the weight gradient on the packed image ----
    dp = r.dx_out[0]
    H2, W2, wb = cfg["H"] // 2, cfg["W"] // 2, cfg["width"]
    dzp = torch.zeros(N, H2 + 2, W2 + 2, wb, dtype=torch.float64)
    for k in range(9):
        rr, ss = divmod(k, 3)
        dzp[:, rr:rr + H2:2, ss:ss + W2:2] += dp.double() * (t["pool_arg"] == k)
    dz0 = dzp[:, 1:H2 + 1, 1:W2 + 1].reshape(-1, wb)
    bn = {k: v.double() for k, v in t["bn1"].items()}
    check_bn_bwd_general(r.d_raw0.reshape(-1, wb), grd("bn1.weight"), grd("bn1.bias"), dz0, t["raw0"].double().reshape(-1, wb), bn["mean"], bn["invstd"], bn["scale"],
                         "stem bn1 backward")
    ximg = r.x.permute(0, 2, 3, 1).contiguous().to(bf16)
    ref, E = wgrad64(ximg, r.d_raw0, 7, 2, 3)
    _assert_within(grd("conv1.weight").double(), ref, E, "stem weight gradient")
    assert same_bits(grd("conv1.weight").contiguous(), r.stem_dw_pad[:, :, :7, :3].contiguous()), "stem weight gradient is not the padded one's [7][7][3] part"
    print_report(r, "backward")


# ---------------------------------------------------------------------------------------------------------------------------------------
# (c) composition, bit for bit
# ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["R1", "R2"])
def test_backward_compositions_agree_bit_for_bit(name):
    r = run(name)
    P, net = r.P, r.net
    _lib, L = _dbg()
    plan = net._last_plan
    dg = r.d_emb.cuda()
    cin0 = P.geo[0]["cin"]
    shape0 = (P.N, P.geo[0]["hin"], P.geo[0]["win"], cin0)
    ranges = [plan.stage_range(s) for s in range(4)]
    assert ranges[0][1] == plan.param_elems and ranges[3][0] == 0
    for s in range(4):
        assert ranges[s][0] < ranges[s][1] and (s == 0 or ranges[s][1] == ranges[s - 1][0])
    fill = lambda: bits(net.flat_grads).fill_(SENTINEL)
    # (1) the whole backward
    fill()
    _lib.check(L.dali_resnet_backward(plan.h, _lib.stream_ptr(), _lib.ptr(dg), 0, 3), "dali_resnet_backward")
    whole, whole_dx = net.flat_grads.cpu(), P.get("grad_cur", bf16, *shape0)
    # every parameter slot is written (the table's segments; what lies between them is padding)
    written = torch.zeros(whole.numel(), dtype=torch.bool)
    for k, (off, numel, _) in P.ptable.items():
        written[off:off + numel] = True
    assert bool((bits(whole)[written] != SENTINEL).all()), "a parameter's gradient slot was not written"
    assert bool(torch.isfinite(whole[written]).all())
    # (2) stage by stage: after stage s its range is final, the ranges of later stages still hold the sentinel
    fill()
    for s in range(4):
        _lib.check(L.dali_resnet_backward(plan.h, _lib.stream_ptr(), _lib.ptr(dg), s, s), "dali_resnet_backward")
        now = net.flat_grads.cpu()
        for s2 in range(s + 1):
            b, e = ranges[s2]
            assert same_bits(now[b:e], whole[b:e]), "after stage %d the range of stage %d is not final" % (s, s2)
        for s2 in range(s + 1, 4):
            b, e = ranges[s2]
            assert bool((bits(now[b:e])[written[b:e]] == SENTINEL).all()), "stage %d wrote into the range of stage %d" % (s, s2)
    assert same_bits(now, whole) and same_bits(P.get("grad_cur", bf16, *shape0), whole_dx)
    # (3) the per-block debug calls
    fill()
    for bi in list(range(len(P.geo) - 1, -1, -1)) + [-1]:
        _lib.check(L.dali_debug_resnet_backward_block(plan.h, _lib.stream_ptr(), _lib.ptr(dg), bi), "dali_debug_resnet_backward_block")
    assert same_bits(net.flat_grads.cpu(), whole) and same_bits(P.get("grad_cur", bf16, *shape0), whole_dx)
    # (4) the snapshot-mode calls (run() made them right after the forward)
    assert same_bits(r.flat, whole) and same_bits(r.dx_out[0], whole_dx)
    # a snapshot buffer that is too small is refused
    snap = torch.zeros(256, dtype=torch.uint8, device="cuda")
    offs = (ctypes.c_int64 * SNAP_COUNT)()
    assert L.dali_debug_resnet_backward_block_snap(plan.h, _lib.stream_ptr(), _lib.ptr(dg), len(P.geo) - 1, _lib.ptr(snap), 256, offs) == DALI_ERR_INVALID
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------------
# (a') the same walk once in eval mode: conv + bn + relu leave the GEMM's fused output stage, the stem runs fused
# ---------------------------------------------------------------------------------------------------------------------------------------
def test_eval_forward_op_by_op():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    cfg = NETS["R1"]
    net, ref, g = make_net(cfg, seed=8)
    net.eval()
    P = Plan(net, cfg)
    N, wb = P.N, cfg["width"]
    x = torch.randn(N, 3, cfg["H"], cfg["W"], generator=g)
    emb = net._run_forward(x.cuda(), False).cpu()
    t = forward_tensors(P, training=False)
    params, buffers = net.flat_params.detach().cpu(), net.flat_buffers.cpu()
    prm = lambda k: P.param(params, k)

    def coeffs(pre, got, what):
        """scale = gamma / sqrt(running_var + eps), shift = beta - running_mean scale in fp32: sqrt, quotient, two products, one sum <= 4u each"""
        sc = prm(pre + ".weight").double() / torch.sqrt(P.buf(buffers, pre + ".running_var").double() + EPS)
        ms = P.buf(buffers, pre + ".running_mean").double() * sc
        sh = prm(pre + ".bias").double() - ms
        _assert_within(got["scale"].double(), sc, 4 * U * sc.abs(), what + " scale")
        _assert_within(got["shift"].double(), sh, 4 * U * (sc.abs() * P.buf(buffers, pre + ".running_mean").double().abs() + sh.abs() + ms.abs()), what + " shift")
        return got["scale"].double(), got["shift"].double()

    def fused(xin, w, stride, pad, s_, h_, idn=None):
        """relu(scale acc + shift (+ identity)) from the fp32 accumulators: the accumulation bound through |scale|, 4u for the stage's terms"""
        u, E = conv64(xin, w, stride, pad)
        z = s_ * u + h_ + (0 if idn is None else idn[0])
        return z.clamp(min=0), s_.abs() * E + 6 * U * ((s_ * u).abs() + h_.abs() + (0 if idn is None else idn[1]))

    # stem: pool0 = bf16(max over the window of scale conv + shift); the convolution's value may be rounded to bf16 before the affine map (the
    # un-fused path stores raw0; the fused one keeps the same rounding point): |scale| (E + HB |u|) either way; max is 1-Lipschitz in the sup norm
    s_, h_ = coeffs("bn1", t["bn1"], "stem bn1")
    ximg = x.permute(0, 2, 3, 1).contiguous().to(bf16)
    u, E = conv64(ximg, prm("conv1.weight").to(bf16), 2, 3)
    z = (s_ * u + h_).permute(0, 3, 1, 2)
    Ez = (s_.abs() * (E + HB * (u.abs() + E)) + 4 * U * ((s_ * u).abs() + h_.abs())).permute(0, 3, 1, 2)
    ref = F.max_pool2d(z, 3, 2, 1).permute(0, 2, 3, 1)
    Emax = F.max_pool2d(Ez, 3, 2, 1).permute(0, 2, 3, 1)
    check_stored(t["pool0"], ref, Emax, "eval pool0")
    xin = t["pool0"]
    for i, gm in enumerate(P.geo):
        b, pre, what = "block%d." % i, gm["name"] + ".", "eval %s " % gm["name"]
        W = lambda c: t[b + "conv%s.w" % c]
        s1, h1 = coeffs(pre + "bn1", t[b + "bn1"], what + "bn1")
        ref, E = fused(xin, W("1"), 1, 0, s1, h1)
        check_stored(t[b + "a1"], ref, E, what + "a1")
        s2, h2 = coeffs(pre + "bn2", t[b + "bn2"], what + "bn2")
        ref, E = fused(t[b + "a1"], W("2"), gm["stride"], 1, s2, h2)
        check_stored(t[b + "a2"], ref, E, what + "a2")
        s3, h3 = coeffs(pre + "bn3", t[b + "bn3"], what + "bn3")
        if gm["has_ds"]:
            assert P.status(b + "wcat") == DALI_ERR_INVALID, "the cat_eval fold is out of this test's scope (needs >= 2 tiles per CU)"
            sd, hd = coeffs(pre + "downsample.1", t[b + "bnd"], what + "bnd")
            ud, Ed = conv64(xin, W("d"), gm["stride"], 0)
            check_stored(t[b + "rawd"], ud, Ed, what + "rawd")
            rd = t[b + "rawd"].double()
            idn = (rd * sd + hd, (rd * sd).abs() + hd.abs())
        else:
            idn = (xin.double(), xin.double().abs())
        ref, E = fused(t[b + "a2"], W("3"), 1, 0, s3, h3, idn)
        check_stored(t[b + "y"], ref, E, what + "y")
        xin = t[b + "y"]
    yl = xin.double().reshape(N, -1, xin.shape[-1])
    HW = yl.shape[1]
    fref = yl.mean(1) + yl.max(1).values
    _assert_within(t["feat"].double(), fref, sum_bound(HW, yl.sum(1)) / HW + 2 * U * fref.abs(), "eval feat")
    rm, rv = P.buf(buffers, "last_bn.running_mean").double(), P.buf(buffers, "last_bn.running_var").double()
    _bn1d_check_y(emb, t["feat"], rm, 1.0 / torch.sqrt(rv + EPS), prm("last_bn.weight"), prm("last_bn.bias"), "eval neck output")
