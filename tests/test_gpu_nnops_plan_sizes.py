"""GPU parity of the memory-bound kernels around the trunk's GEMMs at the BENCHMARKED plan's own sizes (configs[1]: batch 256 of
256 x 128 images; ViT-B at 25216 tokens; the neck at batch 256 and the inference batch 500).

Why beside tests/test_gpu_nnops.py: that file runs these kernels on 27 to 512 pixels, where the reduce pass has one block, the
two-level in-launch reduction (reduce_finish.h) has one level-1 row, no grid-stride loop runs a second iteration and every max-pool
side is even.  At plan sizes the reduction runs with up to 64 level-1 rows (its 8-chain level-1 loop and its 32-, 16-load and tail
level-2 paths), the grid-stride loops wrap, and the non-quad max-pool kernels run for odd stem sides.

Inputs are small integers, power-of-two scales and inverse standard deviations, integer shifts and means: every sum is then exact in
any order, so gradients of gamma / beta, means, masks, pooled values and arg-maxes are compared BIT FOR BIT with integer or fp64
host sums.  Outputs that pass through a rounding step by design (invstd, the folded BatchNorm backward, BatchNorm1d, LayerNorm) are
bounded element-wise by the rounding error of the kernel's own formula, derived next to each bound.  References are computed on the
host in integer or fp64 arithmetic, in chunks (host memory stays at a few GB)."""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from resnet_checks import _assert_within, _bn1d_check_y, _draw_bound_check, _pack_bits, _ulp      # shared with tests/test_gpu_resnet_plan.py
from vit_checks import check_bn1d_bwd, check_layernorm_fwd

pytestmark = pytest.mark.gpu
bf16 = torch.bfloat16
U = 2.0 ** -24                      # fp32 unit roundoff
HB = 2.0 ** -8                      # bf16 unit roundoff (half an ulp, relative)
EPS = float(np.float32(1e-5))       # the BatchNorm eps as the kernels see it (an fp32 argument)
MOM = 0.125                         # power-of-two momentum: (1 - m) * r and m * s are exact, the update is one rounding
CHUNK = 1 << 22                     # host reference chunk (elements of a [rows, C] tensor)


@pytest.fixture(scope="module")
def nn():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from daliid_amd import ops_nn
    torch.set_num_threads(min(16, max(torch.get_num_threads(), 8)))
    return ops_nn


def _gen(*key):
    return torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))


def _ints(lo, hi, shape, gen, dtype=torch.int8):
    return torch.randint(lo, hi + 1, shape, generator=gen, dtype=dtype)


def _pow2(n, gen, lo=-2, hi=1, signed=True):
    """2^k, k in [lo, hi], with random signs"""
    v = 2.0 ** _ints(lo, hi, (n,), gen, torch.int32).double()
    if signed:
        v = v * (1 - 2 * _ints(0, 1, (n,), gen, torch.int32)).double()
    return v.float()


def _dev(t):
    """host integer tensor -> device bf16 (every value used here is exact in bf16)"""
    return t.cuda().to(bf16)


def _rows(P, C):
    return max(1, CHUNK // C)


# ---------------------------------------------------------------------------------------------------------------------------
# 1-3: BatchNorm finalize (reduce_finish_kernel<2, FinBnFwd>)
# ---------------------------------------------------------------------------------------------------------------------------
def _fin_slab(rows, C, seed, m=4):
    """synthetic partial slab [rows, C, 2] of m integer pixels per row: (sum x, sum x^2), integers < 2^24, exact in fp32"""
    g = _gen("fin", rows, C, seed)
    off = _ints(-6, 6, (C,), g)
    x = _ints(-3, 3, (rows, m, C), g) + off
    x[:, :, ::16] = off[::16]                                    # constant channels: variance exactly 0
    xi = x.to(torch.int32)
    slab = torch.stack([xi.sum(1), (xi * xi).sum(1)], -1).float()
    return slab, rows * m


def _fin_params(C, seed):
    g = _gen("finp", C, seed)
    return (_pow2(C, g), _ints(-3, 3, (C,), g).float(), _ints(-4, 4, (C,), g).float(), _ints(1, 6, (C,), g).float())


def _fin_ref(S, count):
    """fp64 reference of FinBnFwd from the exact channel sums S [C, 2]: E[x^2] - mean^2 clamped at 0, unbiased running variance"""
    mean = S[:, 0] / count
    var = np.maximum(S[:, 1] / count - mean * mean, 0.0)
    unb = var * count / (count - 1.0) if count > 1 else var
    return mean, 1.0 / np.sqrt(var + EPS), unb


def _run_fin(nn, slab, count, params):
    gamma, beta, rm, rv = params
    rm_g, rv_g = rm.cuda(), rv.cuda()
    out = nn.bn_finalize(slab, count, gamma.cuda(), beta.cuda(), rm_g, rv_g, momentum=MOM, eps=EPS)
    return out + (rm_g, rv_g)


def _check_fin(out, S, count, params, what):
    gamma, beta, rm0, rv0 = (t.double().numpy() for t in params)
    scale, shift, mean, invstd, rm, rv = (t.cpu().double().numpy() for t in out)
    r_mean, r_inv, r_unb = _fin_ref(S, count)
    assert np.array_equal(mean, r_mean.astype(np.float32).astype(np.float64)), what + ": mean not the fp64 mean rounded to fp32"
    assert (np.abs(invstd - r_inv) <= _ulp(r_inv)).all(), (what, np.abs(invstd - r_inv).max())
    r_sc = gamma * r_inv                                          # gamma a power of two: scale = gamma * invstd carries invstd's error
    assert (np.abs(scale - r_sc) <= _ulp(r_sc)).all(), (what, np.abs(scale - r_sc).max())
    # shift = beta - mean * scale of the (checked) fp32 mean and scale: half an ulp for the product, half an ulp for the difference
    # (whose magnitude is at most |beta| + |p|)
    p = mean * scale
    assert (np.abs(shift - (beta - p)) <= 0.5 * (_ulp(p) + _ulp(np.abs(beta) + np.abs(p)))).all(), what + ": shift"
    for got, r0, s, name in ((rm, rm0, r_mean, "running_mean"), (rv, rv0, r_unb, "running_var")):
        _check_running(got, r0, s, (what, name))


def _check_running(got, r0, s, what):
    """(1 - m) * r + m * fp32(s), m a power of two and r an integer: exact products, so half an ulp of the sum (at most |a| + |b|)
    and m x half an ulp of fp32(s)"""
    a, b = (1 - MOM) * r0, MOM * s
    assert (np.abs(got - (a + b)) <= 0.5 * (_ulp(np.abs(a) + np.abs(b)) + MOM * _ulp(s))).all(), what


FIN_ROWS = [1, 7, 8, 9, 100, 255, 256, 300, 511, 512, 1000, 4096]      # level-1 rows S = 1, 1, 1, 1, 12, 31, 32, 37, 63, 64, 64, 64


@pytest.mark.parametrize("C", [64, 2048])
@pytest.mark.parametrize("rows", FIN_ROWS)
def test_bn_finalize_reduce_levels(nn, rows, C):
    slab, count = _fin_slab(rows, C, 0)
    params = _fin_params(C, 0)
    out = _run_fin(nn, slab.cuda(), count, params)
    _check_fin(out, slab.double().sum(0).numpy(), count, params, "rows %d C %d" % (rows, C))


# ---- 2: the level-1 -> level-2 hand-off under back-to-back launches with different data ----------------------------------------
def _bwd_case(P, C, dual, mask, seed, offset=False):
    """host integer inputs of one bn_bwd call (mask: 'recompute' from scale / shift, 'ymask' from a bf16 y, 'ybits')"""
    g = _gen("bwd", P, C, dual, mask, seed, offset)
    d = {"P": P, "C": C, "mask": mask, "g": _ints(-2, 2, (P, C), g)}
    sides = []
    for _ in range(2 if dual else 1):
        if offset:                                                # raw in [126, 130], mean 128: K - Q * raw cancels
            raw = _ints(126, 130, (P, C), g, torch.int16)
            mean = torch.full((C,), 128.0)
        else:
            raw = _ints(-4, 4, (P, C), g, torch.int16)
            mean = _ints(-1, 1, (C,), g).float()
        invstd = _pow2(C, g, -2, 0, signed=False)
        scale = _pow2(C, g, -1, 1) * invstd
        shift = (_ints(-2, 2, (C,), g).float() - mean * scale) if offset else _ints(-2, 2, (C,), g).float()
        sides.append(dict(raw=raw, mean=mean, invstd=invstd, scale=scale, shift=shift))
    d["sides"] = sides
    a = sides[0]
    if mask == "recompute":
        d["m"] = None                                             # computed per chunk from raw * scale + shift (exact in fp32)
    elif mask == "ymask":
        d["y"] = _ints(-1, 1, (P, C), g)
    else:
        d["m"] = _ints(0, 1, (P, C), g).bool()
    return d


def _bwd_mask(d, i0, i1):
    a = d["sides"][0]
    if d["mask"] == "recompute":
        return (a["raw"][i0:i1].float() * a["scale"] + a["shift"]) > 0
    if d["mask"] == "ymask":
        return d["y"][i0:i1] > 0
    return d["m"][i0:i1]


def _bwd_sums(d):
    """exact per-channel sums: S1 = sum dz, T_k = sum dz * (raw_k - mean_k) (int64)"""
    P, C = d["P"], d["C"]
    S1 = torch.zeros(C, dtype=torch.int64)
    T = [torch.zeros(C, dtype=torch.int64) for _ in d["sides"]]
    step = _rows(P, C)
    for i0 in range(0, P, step):
        i1 = min(P, i0 + step)
        dz = d["g"][i0:i1].to(torch.int32) * _bwd_mask(d, i0, i1)
        S1 += dz.sum(0, dtype=torch.int64)
        for k, s in enumerate(d["sides"]):
            T[k] += (dz * (s["raw"][i0:i1].to(torch.int32) - s["mean"].to(torch.int32))).sum(0, dtype=torch.int64)
    return S1.double().numpy(), [t.double().numpy() for t in T]


def _bwd_dev(d):
    dev = {"g": _dev(d["g"])}
    dev["sides"] = [{k: (_dev(v) if k == "raw" else v.cuda()) for k, v in s.items()} for s in d["sides"]]
    if d["mask"] == "ymask":
        dev["ymask"] = _dev(d["y"])
    elif d["mask"] == "ybits":
        dev["ybits"] = _pack_bits(d["m"]).cuda()
    return dev


def _run_bwd(nn, dev, want_dz=False):
    a = dev["sides"][0]
    side_b = None
    if len(dev["sides"]) > 1:
        b = dev["sides"][1]
        side_b = (b["raw"], b["mean"], b["invstd"], b["scale"])
    return nn.bn_bwd(dev["g"], a["raw"], a["mean"], a["invstd"], a["scale"], a["shift"], ymask=dev.get("ymask"), relu=True,
                     side_b=side_b, want_dz=want_dz, ybits=dev.get("ybits"))


def _check_bwd_sums(out, d, sums, what):
    """dgamma = sum dz * xhat, dbeta = sum dz: exact (integers times a power-of-two invstd)"""
    S1, T = sums
    for k, s in enumerate(d["sides"]):
        dgamma, dbeta = out[3 * k + 1].cpu().double().numpy(), out[3 * k + 2].cpu().double().numpy()
        r_dg = T[k] * s["invstd"].double().numpy()
        assert np.array_equal(r_dg.astype(np.float32), r_dg) and np.array_equal(S1.astype(np.float32), S1), "reference not exact in fp32"
        assert np.array_equal(dbeta, S1), "%s side %d: dbeta off in %d channels" % (what, k, int((dbeta != S1).sum()))
        assert np.array_equal(dgamma, r_dg), "%s side %d: dgamma off in %d channels" % (what, k, int((dgamma != r_dg).sum()))


def test_reduce_finish_handoff_back_to_back(nn):
    """Six launches at one shape, three different data sets twice over, enqueued back to back and only then checked: a level-2 read
    of a stale level-1 row would return another launch's sums.  bn_bwd dual at layer4's 32768 x 2048 runs 25 x 64 = 1600
    workgroups; the finalize slab 16 x 64.  The largest workspace user goes first, so nothing is reallocated in between."""
    bwd = [_bwd_case(32768, 2048, True, "ybits", k) for k in range(3)]
    bwd_dev = [_bwd_dev(d) for d in bwd]
    _run_bwd(nn, bwd_dev[0])                                      # sizes the workspace for everything below
    torch.cuda.synchronize()
    fin = [_fin_slab(4096, 2048, 10 + k) for k in range(3)]
    fin_dev = [s.cuda() for s, _ in fin]
    params = _fin_params(2048, 1)
    fin_out = [_run_fin(nn, fin_dev[k % 3], fin[k % 3][1], params) for k in range(6)]
    bwd_out = [_run_bwd(nn, bwd_dev[k % 3]) for k in range(6)]
    torch.cuda.synchronize()
    for k in range(6):
        slab, count = fin[k % 3]
        _check_fin(fin_out[k], slab.double().sum(0).numpy(), count, params, "finalize launch %d" % k)
    sums = [_bwd_sums(d) for d in bwd]
    for k in range(6):
        _check_bwd_sums(bwd_out[k], bwd[k % 3], sums[k % 3], "bn_bwd launch %d" % k)


# ---- 3: convolution statistics epilogue into finalize ---------------------------------------------------------------------
@pytest.mark.parametrize("case", [(64, 32, 64, 256, 8), (16, 8, 512, 2048, 32)], ids=["layer1_1x1_64-256", "layer4_1x1_512-2048"])
def test_conv_stats_finalize_exact(nn, case):
    """x in {-1, 0, 1}, sparse +-1 weights: the conv output is integer, and with every channel's total sum of squares below 2^24 every
    tile's fp32 partial sums are exact, so the finalized statistics must equal the fp64 statistics of the exact output."""
    h, w, cin, cout, nnz = case
    P = 256 * h * w
    g = _gen("convstats", *case)
    x = _ints(-1, 1, (P, cin), g)
    wt = _ints(-1, 1, (cout, cin), g) * (torch.rand(cout, cin, generator=g) < nnz / cin)
    _, stats = nn.conv2d_fwd(_dev(x).view(256, h, w, cin), _dev(wt).view(cout, 1, 1, cin), 1, 0, want_stats=True)
    wf = wt.float().t().contiguous()
    S = torch.zeros(cout, 2, dtype=torch.float64)
    for i0 in range(0, P, 32768):
        y = x[i0:i0 + 32768].float() @ wf                         # integers, exact in fp32
        S[:, 0] += y.sum(0, dtype=torch.float64)
        S[:, 1] += (y * y).sum(0, dtype=torch.float64)
    assert (S[:, 1] < 2 ** 24).all(), "input ranges must keep every tile's sum of squares exact in fp32"
    params = _fin_params(cout, 3)
    out = _run_fin(nn, stats, P, params)
    _check_fin(out, S.numpy(), P, params, "conv %s" % (case,))


def test_conv_stats_finalize_offset_mean(nn):
    """Channel mean ~100x the standard deviation (layer1's 1x1 64 -> 256): E[x^2] - mean^2 cancels four decimal digits of the fp32
    tile sums.  invstd within 1e-4 relative of a two-pass fp64 reference on the same bf16 inputs; the error at 1000x is printed."""
    h, w, cin, cout = 64, 32, 64, 256
    P = 256 * h * w
    g = _gen("convoffset")
    x = torch.randn(P, cin, generator=g).to(bf16)
    x[:, 0] = 1.0                                                 # constant input channel carries the mean
    x64 = x.double()
    mx = x64.mean(0)
    xc = x64 - mx
    cov = (xc.t() @ xc) / P                                       # two-pass fp64 covariance of the inputs
    del xc, x64
    xg = x.cuda().view(256, h, w, cin)
    for ratio in (100.0, 1000.0):
        wt = (torch.randn(cout, cin, generator=g) / cin ** 0.5).to(bf16)
        wt[:, 0] = ratio                                          # exact in bf16 (100, 1000)
        w64 = wt.double()
        var = ((w64 @ cov) * w64).sum(1)                          # var of y = w . x: w^T cov w
        mean = w64 @ mx
        r_inv = 1.0 / torch.sqrt(var + EPS)
        _, stats = nn.conv2d_fwd(xg, wt.cuda().view(cout, 1, 1, cin), 1, 0, want_stats=True)
        _, _, _, inv = nn.bn_finalize(stats, P, torch.ones(cout).cuda(), torch.zeros(cout).cuda(), eps=EPS)
        rel = ((inv.cpu().double() - r_inv).abs() / r_inv).max().item()
        print("mean / std %.0f (measured %.0f): max relative invstd error %.3g" % (ratio, (mean.abs() / var.sqrt()).median().item(), rel))
        if ratio == 100.0:
            assert rel <= 1e-4, rel


# ---------------------------------------------------------------------------------------------------------------------------
# 4: bn_act (block outputs)
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(524288, 64), (524288, 256), (131072, 512), (32768, 2048), (400000, 96)], ids=lambda s: "%dx%d" % s)
def test_bn_act_plan_sizes(nn, shape):
    """raw, identity, raw2 in [-8, 8], power-of-two scales, integer shifts: every y is a multiple of 1/4 below 64, exact in fp32 and
    bf16, so y and the mask bytes are bit-exact.  (400000, 96): the grid stride is not a multiple of C (no fixed_c) and the 16384-block
    cap makes some threads run a second iteration."""
    P, C = shape
    g = _gen("act", P, C)
    raw, idn, raw2 = (_ints(-8, 8, (P, C), g) for _ in range(3))
    sc, sh, sc2, sh2 = _pow2(C, g), _ints(-4, 4, (C,), g).float(), _pow2(C, g), _ints(-4, 4, (C,), g).float()
    rg, ig, r2g = _dev(raw), _dev(idn), _dev(raw2)
    scg, shg, sc2g, sh2g = sc.cuda(), sh.cuda(), sc2.cuda(), sh2.cuda()
    variants = [("plain", False, False), ("plain", True, True), ("identity", True, True), ("identity", False, True),
                ("raw2", True, True), ("raw2", False, True)]
    step = _rows(P, C)
    for kind, relu, want_mask in variants:
        kw = {"identity": ig} if kind == "identity" else ({"raw2": r2g, "scale2": sc2g, "shift2": sh2g} if kind == "raw2" else {})
        res = nn.bn_act(rg, scg, shg, relu=relu, want_mask=want_mask, **kw)
        y, bits = res if want_mask else (res, None)
        for i0 in range(0, P, step):
            i1 = min(P, i0 + step)
            z = raw[i0:i1].float() * sc + sh
            if kind == "identity":
                z += idn[i0:i1].float()
            elif kind == "raw2":
                z += raw2[i0:i1].float() * sc2 + sh2
            if relu:
                z.clamp_(min=0)
            assert torch.equal(y[i0:i1].cpu(), z.to(bf16)), "%s relu=%d: y differs in rows %d..%d" % (kind, relu, i0, i1)
            if want_mask:
                assert torch.equal(bits[i0 * C // 8:i1 * C // 8].cpu(), _pack_bits(z > 0)), "%s relu=%d: mask rows %d..%d" % (kind, relu, i0, i1)
        del y, bits, res


# ---------------------------------------------------------------------------------------------------------------------------
# 5: BatchNorm backward (single / dual, three mask sources)
# ---------------------------------------------------------------------------------------------------------------------------
def _check_bwd_full(out, d, sums, what):
    _check_bwd_sums(out, d, sums, what)
    P, C = d["P"], d["C"]
    S1, T = sums
    dz_k = out[-1]
    step = _rows(P, C)
    for i0 in range(0, P, step):
        i1 = min(P, i0 + step)
        dz = d["g"][i0:i1].to(torch.int32) * _bwd_mask(d, i0, i1)
        assert torch.equal(dz_k[i0:i1].cpu(), dz.to(bf16)), "%s: dz differs in rows %d..%d" % (what, i0, i1)
        for k, s in enumerate(d["sides"]):
            S2 = torch.from_numpy(T[k]) * s["invstd"].double()
            _draw_bound_check(out[3 * k][i0:i1].cpu(), dz, s["raw"][i0:i1], s["mean"], s["invstd"], s["scale"],
                              torch.from_numpy(S1), S2, P, "%s side %d rows %d..%d" % (what, k, i0, i1))


BWD_SHAPES = [(524288, 64, False), (524288, 256, True), (131072, 128, False), (32768, 2048, True), (65000, 256, False)]


@pytest.mark.parametrize("mask", ["recompute", "ymask", "ybits"])
@pytest.mark.parametrize("shape", BWD_SHAPES, ids=lambda s: "%dx%d%s" % (s[0], s[1], "_dual" if s[2] else ""))
def test_bn_bwd_plan_sizes(nn, shape, mask):
    P, C, dual = shape
    d = _bwd_case(P, C, dual, mask, 0)
    out = _run_bwd(nn, _bwd_dev(d), want_dz=True)
    _check_bwd_full(out, d, _bwd_sums(d), "bn_bwd %dx%d dual=%d %s" % (P, C, dual, mask))


def test_bn_bwd_offset_raw(nn):
    """raw in [126, 130] around mean 128: the folded K - Q*raw cancels; the bound charges Q*raw's rounding, not the result's"""
    d = _bwd_case(131072, 128, False, "recompute", 0, offset=True)
    out = _run_bwd(nn, _bwd_dev(d), want_dz=True)
    _check_bwd_full(out, d, _bwd_sums(d), "bn_bwd offset")


# ---------------------------------------------------------------------------------------------------------------------------
# 6: stem max-pool with its BatchNorm
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(256, 128, 64, 64), (256, 63, 33, 64)], ids=["128x64_quads", "63x33_odd"])
def test_maxpool_bn_plan_sizes(nn, shape):
    """raw in {-2..2} (ties in nearly every window), power-of-two scales of both signs, integer shifts: z = raw*scale + shift is exact,
    so the pooled output and the arg-max (first maximum in row-major window order, unfold + argmax's documented tie rule) are
    bit-exact; the backward's dgamma / dbeta are exact integer sums, draw meets the bound of _draw_bound_check."""
    N, H, W, C = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    g = _gen("maxpool", *shape)
    raw = _ints(-2, 2, (N, H, W, C), g)
    mean = _ints(-1, 1, (C,), g).float()
    invstd = _pow2(C, g, -2, 0, signed=False)
    scale = _pow2(C, g, -1, 1) * invstd                       # negative gammas -> negative scales
    shift = _ints(-2, 2, (C,), g).float()
    rg = _dev(raw)
    out, arg = nn.maxpool_bn_fwd(rg, scale.cuda(), shift.cuda())
    NB = 16
    for n0 in range(0, N, NB):
        z = (raw[n0:n0 + NB].float() * scale + shift).permute(0, 3, 1, 2)
        cols = F.unfold(F.pad(z, (1, 1, 1, 1), value=float("-inf")), 3, stride=2).view(z.shape[0], C, 9, Ho * Wo)
        a = cols.argmax(2)
        m = cols.gather(2, a.unsqueeze(2)).squeeze(2)
        to_nhwc = lambda t: t.view(z.shape[0], C, Ho, Wo).permute(0, 2, 3, 1)
        assert torch.equal(out[n0:n0 + NB].cpu(), to_nhwc(m).to(bf16)), "pooled values differ in images %d.." % n0
        assert torch.equal(arg[n0:n0 + NB].cpu(), to_nhwc(a).to(torch.uint8)), "arg differs in images %d.." % n0
    del out
    # backward: dz scattered through the (verified) arg-max taps
    dp = _ints(-2, 2, (N, Ho, Wo, C), g)
    draw, dg, db = nn.maxpool_bn_bwd(_dev(dp), arg, rg, mean.cuda(), invstd.cuda(), scale.cuda())
    argc = arg.cpu()
    del arg, rg
    dz = torch.empty(N, H, W, C, dtype=torch.int8)
    for n0 in range(0, N, NB):
        n1 = min(N, n0 + NB)
        dzp = torch.zeros(n1 - n0, H + 2, W + 2, C, dtype=torch.int8)
        for k in range(9):
            r, s = divmod(k, 3)
            dzp[:, r:r + 2 * Ho:2, s:s + 2 * Wo:2] += dp[n0:n1] * (argc[n0:n1] == k)
        dz[n0:n1] = dzp[:, 1:H + 1, 1:W + 1]
    dz2, raw2 = dz.view(-1, C), raw.view(-1, C)
    P = dz2.shape[0]
    S1 = torch.zeros(C, dtype=torch.int64)
    T = torch.zeros(C, dtype=torch.int64)
    step = _rows(P, C)
    for i0 in range(0, P, step):
        dzi = dz2[i0:i0 + step].to(torch.int32)
        S1 += dzi.sum(0, dtype=torch.int64)
        T += (dzi * (raw2[i0:i0 + step].to(torch.int32) - mean.to(torch.int32))).sum(0, dtype=torch.int64)
    S1, S2 = S1.double(), T.double() * invstd.double()
    assert torch.equal(db.cpu().double(), S1) and torch.equal(dg.cpu().double(), S2), "maxpool bwd dgamma / dbeta not exact"
    draw2 = draw.view(-1, C)
    for i0 in range(0, P, step):
        _draw_bound_check(draw2[i0:i0 + step].cpu(), dz2[i0:i0 + step], raw2[i0:i0 + step], mean, invstd, scale, S1, S2, P,
                          "maxpool draw rows %d.." % i0)


# ---------------------------------------------------------------------------------------------------------------------------
# 7: head GAP + GMP pool
# ---------------------------------------------------------------------------------------------------------------------------
def _head_check_fwd(nn, x, N, h, w, C, mode):
    HW = h * w
    f, arg = nn.head_pool_fwd(_dev(x).view(N, h, w, C), mode)
    xv = x.view(N, HW, C)
    ra = xv.argmax(1)                                             # first maximum: the lowest pixel index wins ties
    mx = xv.gather(1, ra.unsqueeze(1)).squeeze(1).double()
    avg = (xv.sum(1, dtype=torch.int32).double() / HW).float().double()  # fp32 quotient, correctly rounded (53 >= 2 * 24 + 2)
    ref = {"both": avg + mx, "gap": avg, "gmp": mx}[mode].float()     # the sum of two fp32 values is exact in fp64: one rounding
    assert torch.equal(f.cpu(), ref), "%s: f differs in %d places" % (mode, int((f.cpu() != ref).sum()))
    assert torch.equal(arg.cpu(), ra.to(torch.int16)), "%s: arg differs" % mode
    return arg, ra


def _head_check_bwd(nn, arg, ra, N, h, w, C, mode, g):
    """dx = df/HW (not gmp) + df at the arg-max pixel (not gap), fp32 then bf16: within one bf16 rounding of the fp64 value plus the
    fp32 rounding of the quotient and the sum (2u(|df/HW| + |dx|))"""
    HW = h * w
    df = torch.randn(N, C, generator=g)
    dx = nn.head_pool_bwd(df.cuda(), arg, (h, w), mode).view(N, HW, C)
    NB = max(1, CHUNK // (HW * C))
    for n0 in range(0, N, NB):
        d = df[n0:n0 + NB].double().unsqueeze(1)
        avg = (d / HW).expand(-1, HW, -1) if mode != "gmp" else torch.zeros(d.shape[0], HW, C, dtype=torch.float64)
        hit = (torch.arange(HW).view(1, HW, 1) == ra[n0:n0 + NB].unsqueeze(1)) if mode != "gap" else torch.zeros(1, 1, 1, dtype=torch.bool)
        ref = avg + hit * d
        _assert_within(dx[n0:n0 + NB].cpu().double(), ref, HB * ref.abs() + (1 + HB) * 2 * U * (avg.abs() + ref.abs()),
                       "head dx %s images %d.." % (mode, n0))


@pytest.mark.parametrize("mode", ["both", "gap", "gmp"])
def test_head_pool_plan_batch(nn, mode):
    N, h, w, C = 256, 16, 8, 2048
    g = _gen("head", mode)
    x = _ints(-3, 3, (N, h * w, C), g)
    arg, ra = _head_check_fwd(nn, x, N, h, w, C, mode)
    _head_check_bwd(nn, arg, ra, N, h, w, C, mode, g)


def test_head_pool_inference_batch(nn):
    g = _gen("head500")
    _head_check_fwd(nn, _ints(-3, 3, (500, 128, 2048), g), 500, 16, 8, 2048, "both")


@pytest.mark.parametrize("mode", ["both", "gap"])
def test_head_pool_non_pow2_hw(nn, mode):
    """24 x 12 = 288 pixels: the fp32 quotient by HW is a real division (the power-of-two path multiplies by 1/HW)"""
    N, h, w, C = 64, 24, 12, 2048
    g = _gen("head288", mode)
    x = _ints(-3, 3, (N, h * w, C), g)
    arg, ra = _head_check_fwd(nn, x, N, h, w, C, mode)
    _head_check_bwd(nn, arg, ra, N, h, w, C, mode, g)


def test_head_pool_hw_limit(nn):
    """arg is int16: HW = 32767 is the largest accepted (the last pixel's index still fits), 32768 is refused"""
    from daliid_amd._lib import DaliError
    x = torch.zeros(1, 32767, 1, 8, dtype=bf16)
    x[0, -1] = 1.0
    x[0, 5] = 1.0 * (torch.arange(8) % 2 == 0)                      # even channels: a tie, the lower index wins
    f, arg = nn.head_pool_fwd(x.cuda())
    expect = torch.where(torch.arange(8) % 2 == 0, 5, 32766).to(torch.int16)
    assert torch.equal(arg.cpu()[0], expect)
    top = [float(np.float32(np.float32(k / 32767) + np.float32(1.0))) for k in (2.0, 1.0)]
    assert torch.equal(f.cpu()[0], torch.where(torch.arange(8) % 2 == 0, top[0], top[1]))
    with pytest.raises(DaliError):
        nn.head_pool_fwd(torch.zeros(1, 32768, 1, 8, dtype=bf16).cuda())


# ---------------------------------------------------------------------------------------------------------------------------
# 8: BatchNorm1d neck
# ---------------------------------------------------------------------------------------------------------------------------
def _bn1d_inputs(N, C, key):
    g = _gen("bn1d", N, C, key)
    off = (torch.rand(C, generator=g) * 2 + 1) * torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
    x = torch.randn(N, C, generator=g) * 2 + off
    gamma = (torch.rand(C, generator=g) + 0.5) * torch.where(torch.rand(C, generator=g) < 0.3, -1.0, 1.0)
    beta = torch.randn(C, generator=g)
    rm, rv = _ints(-2, 2, (C,), g).float(), _ints(1, 6, (C,), g).float()     # integers: (1 - MOM) * r is exact
    return g, x, gamma, beta, rm, rv


@pytest.mark.parametrize("shape", [(256, 2048), (37, 2040)], ids=["256x2048", "37x2040_ragged"])
def test_bn1d_train_plan_sizes(nn, shape):
    N, C = shape
    g, x, gamma, beta, rm, rv = _bn1d_inputs(N, C, "train")
    rm_g, rv_g = rm.cuda(), rv.cuda()
    y, mean, invstd = nn.bn1d_fwd(x.cuda(), gamma.cuda(), beta.cuda(), rm_g, rv_g, training=True, momentum=MOM, eps=EPS)
    xd = x.double()
    m64 = xd.mean(0)
    v = ((xd - m64) ** 2).sum(0)
    i64 = 1.0 / torch.sqrt(v / N + EPS)
    mk, ik = mean.cpu().double(), invstd.cpu().double()
    _assert_within(mk, m64, torch.from_numpy(_ulp(m64.numpy())), "bn1d mean")
    _assert_within(ik, i64, torch.from_numpy(_ulp(i64.numpy())), "bn1d invstd")
    _bn1d_check_y(y, x, m64, i64, gamma, beta, "bn1d train y")
    for got, r0, s, name in ((rm_g, rm, m64, "running_mean"), (rv_g, rv, v / (N - 1), "running_var")):
        _check_running(got.cpu().double().numpy(), r0.double().numpy(), s.numpy(), name)
    # backward, from the kernel's own mean / invstd
    dy = torch.randn(N, C, generator=g)
    dx, dg, db = nn.bn1d_bwd(x.cuda(), dy.cuda(), gamma.cuda(), mean, invstd)
    check_bn1d_bwd(dx.cpu(), dg.cpu(), db.cpu(), x, dy, gamma, mk, ik)                 # shared with tests/test_gpu_vit_plan.py


@pytest.mark.parametrize("shape", [(500, 2048), (37, 2040)], ids=["500x2048", "37x2040_ragged"])
def test_bn1d_eval_plan_sizes(nn, shape):
    N, C = shape
    _, x, gamma, beta, rm, rv = _bn1d_inputs(N, C, "eval")
    y, mean, invstd = nn.bn1d_fwd(x.cuda(), gamma.cuda(), beta.cuda(), rm.cuda(), rv.cuda(), training=False, eps=EPS)
    i64 = 1.0 / torch.sqrt(rv.double() + EPS)
    assert torch.equal(mean.cpu(), rm)
    _assert_within(invstd.cpu().double(), i64, 3 * U * i64, "bn1d eval invstd")
    _bn1d_check_y(y, x, rm.double(), i64, gamma, beta, "bn1d eval y")


# ---------------------------------------------------------------------------------------------------------------------------
# 9: ViT LayerNorm at the plan size (batch 32 x 788 tokens, width 768)
# ---------------------------------------------------------------------------------------------------------------------------
def test_layernorm_bwd_vit_plan_size(nn):
    """integer x and g, integer row means and power-of-two rstd, power-of-two gamma: xhat and g*gamma are exact, so dgamma / dbeta
    (the reduce_finish sums over 485 row blocks: its 32-, 16-load and tail level-2 paths) are bit-exact; in dx the row means of
    g*gamma and g*gamma*xhat are exact sums divided by C (1u each), then xh*s2 and the two subtractions (1u each), the power-of-two
    rstd exact: |o - dx64| <= 4u |rstd|(|g gamma| + |s1| + |xh s2|), and one bf16 rounding."""
    from daliid_amd import ops_vit
    rows, C = 25216, 768
    g = _gen("lnbwd")
    x, gr = _ints(-8, 8, (rows, C), g), _ints(-2, 2, (rows, C), g)
    mu = _ints(-2, 2, (rows,), g).float()
    rs = _pow2(rows, g, -2, 0, signed=False)
    gamma = _pow2(C, g, -1, 1)
    dx, dg, db = ops_vit.layernorm_bwd(_dev(gr), _dev(x), gamma.cuda(), mu.cuda(), rs.cuda())
    xh = (x.double() - mu.double().unsqueeze(1)) * rs.double().unsqueeze(1)
    gd = gr.double()
    assert torch.equal(db.cpu().double(), gd.sum(0)), "LayerNorm dbeta not exact"
    assert torch.equal(dg.cpu().double(), (gd * xh).sum(0)), "LayerNorm dgamma not exact"
    gh = gd * gamma.double()
    s1, s2 = gh.mean(1, keepdim=True), (gh * xh).mean(1, keepdim=True)
    ref = rs.double().unsqueeze(1) * (gh - s1 - xh * s2)
    E = 4 * U * rs.double().unsqueeze(1) * (gh.abs() + s1.abs() + (xh * s2).abs())
    _assert_within(dx.cpu().double(), ref, HB * ref.abs() + (1 + HB) * E, "LayerNorm dx")


def test_layernorm_fwd_vit_plan_size(nn):
    """mean: a per-lane sequential sum (<= 16 terms) and a 6-level butterfly, then / C: <= 24u sum|x| / C + 1 ulp;  rstd: the same
    sums of squares of (x - mean) + eps, sqrtf and the reciprocal: <= 32u relative;  y = (x - mean) * rstd * gamma + beta in fp32
    then bf16: one bf16 rounding plus the propagated mean / rstd errors and 4u of the terms."""
    from daliid_amd import ops_vit
    rows, C = 25216, 768
    g = _gen("lnfwd")
    x = (torch.randn(rows, C, generator=g) + torch.randn(rows, 1, generator=g)).to(bf16)
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    eps = float(np.float32(1e-6))
    y, mean, rstd = ops_vit.layernorm_fwd(x.cuda(), gamma.cuda(), beta.cuda(), eps=eps)
    check_layernorm_fwd(y.cpu(), mean.cpu(), rstd.cpu(), x, gamma, beta, eps)          # the bound above, shared with tests/test_gpu_vit_plan.py
