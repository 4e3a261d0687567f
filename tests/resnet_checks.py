"""Checks shared by tests/test_gpu_nnops_plan_sizes.py (the BatchNorm / pooling kernels on their own, exact operands) and
tests/test_gpu_resnet_plan.py (the same kernels as the ResNet plan launches them, on the plan's own tensors): one derivation, one bound.
The first part was moved here from test_gpu_nnops_plan_sizes.py unchanged; the second part restates the same derivations for general
(not power-of-two, not integer) operands, every extra rounding charged where it happens.  The third part holds the inference forward's ops
(tests/test_gpu_resnet_eval_plan.py on the plan's tensors, tests/test_resnet_eval_twin_cpu.py on an explicit twin's)."""
import numpy as np
import torch

U = 2.0 ** -24                      # fp32 unit roundoff
U1 = 2.0 ** -23                     # one fp32 rounding of a partial sum, relative to the sum of magnitudes
HB = 2.0 ** -8                      # bf16 unit roundoff (half an ulp, relative)


# ---------------------------------------------------------------------------------------------------------------------------
# moved from tests/test_gpu_nnops_plan_sizes.py (assertions unchanged)
# ---------------------------------------------------------------------------------------------------------------------------
def _pack_bits(b):
    """bool [.., 8k] -> bytes: bit t of byte i = b.flatten()[8i + t] (the kernels' mask layout)"""
    w = torch.tensor([1, 2, 4, 8, 16, 32, 64, 128], dtype=torch.uint8, device=b.device)
    return (b.reshape(-1, 8).to(torch.uint8) * w).sum(1, dtype=torch.uint8)


def _ulp(a):
    """fp32 ulp of |a| (float64 numpy in and out)"""
    return np.spacing(np.abs(np.asarray(a, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def _assert_within(got, ref, bound, what):
    err = (got - ref).abs()
    bad = err > bound
    if bad.any():
        i = int(torch.argmax((err - bound).flatten()))
        raise AssertionError("%s: %d elements off; worst at %d: got %r, ref %r, bound %r" % (
            what, int(bad.sum()), i, float(got.flatten()[i]), float(ref.flatten()[i]), float(bound.flatten()[i])))


def _draw_bound_check(got, dz, raw, mean, invstd, scale, S1, S2, N, what):
    """draw against the unfolded fp64 formula  scale * (dz - S1/N - xhat * S2/N),  xhat = (raw - mean) * invstd.
    The kernel computes the folded form  o = A*dz + K - Q*raw  (FinBnBwd: A = scale, Q = fp32(scale*invstd*S2/N),
    K = fp32(Q64*mean - scale*S1/N), both rounded once from fp64), in fp32 without contraction, then rounds o to bf16:
      A*dz exact (power-of-two scale, integer dz);  rounding K, Q: u|K|, u|Q*raw|;  the add: u(|A dz| + |K|);
      Q*raw: u|Q*raw|;  the subtraction: u(|A dz| + |K| + |Q raw|)   ->  |o - draw64| <= E = 2u(|A dz| + 2|K| + 2|Q raw|)
      bf16(o): within HB|o| <= HB(|draw64| + E)                 ->  |out - draw64| <= HB|draw64| + (1 + HB) E"""
    scale64 = scale.double()
    q = scale64 * invstd.double() * (S2 / N)
    K = q * mean.double() - scale64 * (S1 / N)
    dzd = dz.double()
    rawd = raw.double()
    ref = scale64 * (dzd - S1 / N - (rawd - mean.double()) * invstd.double() * (S2 / N))
    E = 2 * U * ((scale64 * dzd).abs() + 2 * K.abs() + 2 * (q * rawd).abs())
    _assert_within(got.double(), ref, HB * ref.abs() + (1 + HB) * E, what)


def _bn1d_check_y(y, x, mean, inv, gamma, beta, what):
    """y = x*sc + sh, sc = fp32(gamma*invstd), sh = fp32(beta - mean*sc): counting the roundings of invstd (<= 2.5u in eval, 1u in
    training), sc, mean, both products, sh and the sum gives <= 8u (|x sc| + |mean sc| + |beta|)"""
    sc = gamma.double() * inv
    ref = x.double() * sc + (beta.double() - mean * sc)
    _assert_within(y.cpu().double(), ref, 8 * U * ((x.double() * sc).abs() + (mean * sc).abs() + beta.double().abs()), what)


# ---------------------------------------------------------------------------------------------------------------------------
# the same derivations for general operands (tests/test_gpu_resnet_plan.py)
# ---------------------------------------------------------------------------------------------------------------------------
def assert_within(got, ref, bound, what):
    """as _assert_within, with NaN counted as off (tests/vit_checks.py)"""
    from vit_checks import assert_within as aw
    aw(got, ref, bound, what)


def ulp32(a):
    """fp32 ulp of |a|, torch float64 in and out"""
    return torch.from_numpy(_ulp(a.detach().numpy()))


def halfulp_bf16(a):
    """half a bf16 ulp at magnitude |a| (float64)"""
    _, e = torch.frexp(a.abs().clamp_min(2.0 ** -126))
    return torch.ldexp(torch.ones_like(a), e.to(a.dtype) - 9)


def sum_bound(terms, mag):
    """fp32 accumulation of `terms` products in any order (inside the MFMAs, across k-tiles, across split-K slabs and their fixed-order
    reduction): every one of at most `terms` partial sums is bounded by the sum of magnitudes `mag` and rounds once (2^-23 of it), two spare
    for an output stage"""
    return (terms + 2) * U1 * mag


def check_stored(got, ref, E, what):
    """a bf16 store of an fp32 value within E of ref: half a bf16 ulp at |ref| + E, plus E"""
    assert_within(got.double(), ref, halfulp_bf16(ref.abs() + E) + E, what)


def check_bn_bwd_general(draw, dgamma, dbeta, dz, raw, mean, invstd, scale, what):
    """launch_bn_bwd on general operands, against fp64 from the plan's own mean / invstd / scale (float64 [C]), dz and raw float64 [P][C]
    (dz = the gradient after the ReLU mask).  Returns nothing; asserts dbeta, dgamma and draw.
      dbeta = S1 = sum dz, dgamma = S2 = sum dz xhat, xhat = fp32((raw - mean) * invstd) (2u per term), summed in fp32 partials finished in a
      fixed order: sum_bound(P) of the magnitudes, + 2u per term of S2, + the final rounding (1 ulp);
      draw: _draw_bound_check's derivation, where now A dz rounds too (general scale: + u|A dz|, inside the same 2u budget doubled: 4u) and the
      kernel's S1 / S2 are its own sums, off by dS1 / dS2 above: + |scale| (dS1 + |xhat| dS2) / P"""
    P = dz.shape[0]
    xh = (raw - mean) * invstd
    S1, S2 = dz.sum(0), (dz * xh).sum(0)
    dS1 = sum_bound(P, dz.abs().sum(0)) + ulp32(S1)
    dS2 = sum_bound(P, (dz * xh).abs().sum(0)) + 2 * U * (dz * xh).abs().sum(0) + ulp32(S2)
    assert_within(dbeta.double(), S1, dS1, what + " dbeta")
    assert_within(dgamma.double(), S2, dS2, what + " dgamma")
    q = scale * invstd * (S2 / P)
    K = q * mean - scale * (S1 / P)
    ref = scale * (dz - S1 / P - xh * (S2 / P))
    E = 4 * U * ((scale * dz).abs() + 2 * K.abs() + 2 * (q * raw).abs()) + scale.abs() * (dS1 + xh.abs() * dS2) / P
    assert_within(draw.double(), ref, HB * ref.abs() + (1 + HB) * E, what + " d(raw)")


def rel_l2(a, b):
    a, b = a.double().flatten(), b.double().flatten()
    return float((a - b).norm() / b.norm().clamp(min=1e-30))


def check_twin_relative(got, twin, ref, floor, what, report):
    """A cancellation-prone quantity (no a-priori bound): the HIP value may sit at most 2 x as far from the fp64 reference as the rounding-matched
    twin's same op on the same inputs, plus `floor` (the derived bound of the quantity's straightforward form, as a rel-L2 figure).  Both figures
    are printed and kept in `report`."""
    e_hip, e_twin = rel_l2(got, ref), rel_l2(twin, ref)
    report.append((what, e_hip, e_twin, floor))
    assert e_hip <= 2 * e_twin + floor, "%s: HIP %.3e from fp64, twin %.3e, floor %.3e (bound %.3e)" % (what, e_hip, e_twin, floor, 2 * e_twin + floor)


# ---------------------------------------------------------------------------------------------------------------------------
# the inference forward, op by op (tests/test_gpu_resnet_eval_plan.py on the plan's tensors, tests/test_resnet_eval_twin_cpu.py on an explicit
# twin's): one function per op kind, each from the op's own STORED operands.  Layouts are the plan's: activations [N][H][W][C] bf16, weight
# images [cout][r][s][cin] bf16, coefficient vectors fp32 [C].  Each function returns (ref, E): the fp64 value of what is stored and how far the
# fp32 value in front of the one bf16 store may sit from it; `stored_bound` adds that store.
# ---------------------------------------------------------------------------------------------------------------------------
import torch.nn.functional as F                                     # noqa: E402

bf16 = torch.bfloat16


def gamma(n):
    """n fp32 roundings in a row: each intermediate is within gamma(n) = n u / (1 - n u) of the exact value of its terms' magnitudes"""
    return n * U / (1.0 - n * U)


def stored_bound(ref, E):
    """check_stored's bound"""
    return halfulp_bf16(ref.abs() + E) + E


def stored_ratio(got, ref, E):
    """the largest |got - ref| over check_stored's bound (NaN -> inf)"""
    r = ((got.double() - ref).abs() / stored_bound(ref, E)).nan_to_num(nan=float("inf"))
    return float(r.max())


def check_stored_report(got, ref, E, what, kind, report):
    """check_stored, the worst error / bound ratio kept under `kind` in `report` (a dict) first"""
    report[kind] = max(report.get(kind, 0.0), stored_ratio(got, ref, E))
    check_stored(got, ref, E, what)


def conv64c(x, w, stride, pad, chunk=32):
    """fp64 convolution of x [N][H][W][cin] with w [cout][r][s][cin] and the same of the magnitudes, [N][Ho][Wo][cout]: a 1x1 as one matrix
    product, anything else by F.conv2d over `chunk` images at a time"""
    co, r, s, ci = w.shape
    if r == 1 and s == 1 and pad == 0:
        xs = x[:, ::stride, ::stride].double()
        w2 = w.reshape(co, ci).double()
        return xs @ w2.t(), xs.abs() @ w2.abs().t()
    # (the patches of `chunk` images as rows of one matrix product: per-image products of a 6 x 2 map would be bound by reading the weights)
    w2 = w.permute(0, 3, 1, 2).reshape(co, ci * r * s).double()                       # unfold's column order: [cin][r][s]
    wa = w2.abs()
    ho, wo = (x.shape[1] + 2 * pad - r) // stride + 1, (x.shape[2] + 2 * pad - s) // stride + 1
    u, mag = [], []
    for n0 in range(0, x.shape[0], chunk):
        xd = x[n0:n0 + chunk].permute(0, 3, 1, 2).double()
        cols = F.unfold(xd, (r, s), padding=pad, stride=stride).transpose(1, 2)       # [n][ho wo][cin r s]
        u.append((cols @ w2.t()).view(-1, ho, wo, co))
        mag.append((cols.abs() @ wa.t()).view(-1, ho, wo, co))
    return torch.cat(u).contiguous(), torch.cat(mag).contiguous()


def eval_conv(x, w, stride, pad):
    """a stored raw convolution (raw0 of the un-fused stem, rawd): the accumulation of K = r s cin products"""
    u, mag = conv64c(x, w, stride, pad)
    return u, sum_bound(w[0].numel(), mag)


def eval_conv_act(x, w, stride, pad, scale, shift, relu=True):
    """a1 / a2 of the inference forward: relu(acc * scale + shift) in the GEMM's output stage (conv.hip OutStage::pre, steps 1 and 8: one
    product, one sum, the maximum exact -> a term passes 2 fp32 roundings)"""
    u, Eacc = eval_conv(x, w, stride, pad)
    s, h = scale.double(), shift.double()
    z = s * u + h
    E = s.abs() * Eacc + gamma(2) * (s.abs() * (u.abs() + Eacc) + h.abs())
    return (z.clamp(min=0) if relu else z), E


def eval_y(a2, w3, s3, h3, res, res_scale=None, bias=None):
    """y of a block that is not folded: relu(acc3 * scale3 + shift3 (+ bias) + (res_scale *) res).  The general output stage (conv.hip
    OutStage::run) forms acc * scale, + shift, + bias, res * res_scale, + that: 4 roundings on the longest path (3 without a branch: product, shift,
    residual); the persistent kernel (fused1x1.h) adds shift + bias once and uses two fused multiply-adds: 3 (2).  The larger count is charged."""
    u, Eacc = eval_conv(a2, w3, 1, 0)
    s, h, r = s3.double(), h3.double(), res.double()
    n = 3
    if res_scale is not None:
        b = bias.double()
        idn, idn_mag, n = r * res_scale.double() + b, (r * res_scale.double()).abs() + b.abs(), 4
    else:
        idn, idn_mag = r, r.abs()
    z = s * u + h + idn
    E = s.abs() * Eacc + gamma(n) * (s.abs() * (u.abs() + Eacc) + h.abs() + idn_mag)
    return z.clamp(min=0), E


def eval_y_folded(a2, x, wcat, shcat):
    """y of the folded first block: relu([a2 | a2 | x | x] . [W3 hi | W3 lo | Wd hi | Wd lo]^T + shcat) from the plan's own image and summed
    shift: 2 (w + cin) products in the accumulators, then ONE fused multiply-add (acc * 1 + shcat, fused1x1.h): 1 rounding"""
    w_, ci = a2.shape[-1], x.shape[-1]
    a, xi, wc = a2.double().reshape(-1, w_), x.double().reshape(-1, ci), wcat.double()
    assert wc.shape[1] == 2 * (w_ + ci)
    cat = torch.cat((a, a, xi, xi), 1)
    u = cat @ wc.t()
    Eacc = sum_bound(2 * (w_ + ci), cat.abs() @ wc.abs().t())
    h = shcat.double()
    E = Eacc + gamma(1) * (u.abs() + Eacc + h.abs())
    return (u + h).clamp(min=0).reshape(a2.shape[:-1] + (wc.shape[0],)), E.reshape(a2.shape[:-1] + (wc.shape[0],))


def stem_conv(ximg, w_stem):
    """the stem convolution from the plan's packed operands: ximg [N][H + 6][W + 8][4] (3 zero pixels in front, a zero 4th channel), w_stem
    [C][7][8][4] (a zero 8th tap, a zero 4th channel): stride 2, no further padding, over the first W + 6 columns; 147 products that are not 0"""
    W6 = ximg.shape[2] - 2
    u, mag = conv64c(ximg[:, :, :W6], w_stem[:, :, :7], 2, 0)
    return u, sum_bound(147, mag)


def pool3x3s2(z, pad_value=float("-inf")):
    """3x3 / stride 2 / pad 1 maximum of z [N][H][W][C] over the real positions of a window (pad_value = -inf)"""
    zp = F.pad(z.permute(0, 3, 1, 2), (1, 1, 1, 1), value=pad_value)
    return F.max_pool2d(zp, 3, 2, 0).permute(0, 2, 3, 1).contiguous()


def eval_stem_pool(u, Eacc, scale, shift):
    """pool0 of the fused stem (stem.hip): the accumulator is rounded to bf16 first (the tile of the five convolution rows holds bf16 keys: HB of
    it -- the issue's derivation took the affine map on the fp32 accumulators; the kernel, the un-fused path and the oracle's twin all round
    here, so the rounding is counted), the maximum is taken over the window's real positions, bn1's product and sum act on the selected element
    (2 roundings).  max is 1-Lipschitz in the sup norm: the bound of a window is the largest of its positions'.  Rounding is monotone: the one
    store of the maximum is the maximum of the stores.  -> (ref, E, border windows whose maximum lies below -(bound): a pool that pads with 0
    cannot pass there)"""
    s, h = scale.double(), shift.double()
    z = s * u + h
    Ez = s.abs() * (Eacc + HB * (u.abs() + Eacc)) + gamma(2) * (s.abs() * (u.abs() + Eacc) * (1 + HB) + h.abs())
    ref, E = pool3x3s2(z), pool3x3s2(Ez, 0.0)
    border = torch.zeros(ref.shape[1], ref.shape[2], dtype=torch.bool)
    border[0, :] = True
    border[:, 0] = True
    negative = (ref + stored_bound(ref, E) < 0) & border.view(1, ref.shape[1], ref.shape[2], 1)
    return ref, E, negative


def stem_pool_exact(raw0, scale, shift):
    """pool0 of the un-fused stem, bit for bit (maxpool_bn_fwd_kernel): z = raw0 * scale + shift in fp32 (product, then sum: the library is built
    without contraction), the maximum over the window's real positions, one bf16 rounding"""
    return pool3x3s2(raw0.float() * scale + shift).to(bf16)


def eval_feat(y, mode):
    """the head pool of the last y [N][h][w][C] (head_pool_fwd_kernel): mean = fp32 sum of HW values >= 0, one quotient; + the maximum: one
    sum.  gmp: the maximum alone, exact.  -> (ref, bound)"""
    yl = y.double().reshape(y.shape[0], -1, y.shape[-1])
    HW = yl.shape[1]
    mean, mx = yl.mean(1), yl.max(1).values
    dmean = sum_bound(HW, yl.abs().sum(1)) / HW
    if mode == "gmp":
        return mx, torch.zeros_like(mx)
    if mode == "gap":
        return mean, dmean + gamma(1) * (mean.abs() + dmean)
    return mean + mx, dmean + gamma(2) * (mean.abs() + dmean + mx.abs())


def check_neck_eval(emb, feat, gamma_, beta, rm, rv, what, eps=float(np.float32(1e-5))):
    """the neck by running statistics: _bn1d_check_y's eval-mode count (invstd <= 2.5u)"""
    _bn1d_check_y(emb, feat, rm.double(), 1.0 / torch.sqrt(rv.double() + eps), gamma_, beta, what)


def eval_check_stem(t, report, what=""):
    """ximg / w_stem -> (raw0 ->) pool0.  With "raw0" in t the un-fused stem: raw0 a stored convolution, pool0 bit for bit the pool kernel's
    formula on the stored raw0; without it the fused stem: pool0 against fp64 from the packed operands (eval_stem_pool).  Either way the
    reference must hold border windows with a negative maximum (returned: how many)."""
    u, Eacc = stem_conv(t["ximg"], t["w_stem"])
    ref, E, negative = eval_stem_pool(u, Eacc, t["bn1.scale"], t["bn1.shift"])
    assert int(negative.sum()) > 0, what + "no border window of the reference has a negative maximum: a pool that pads with 0 would pass"
    if "raw0" in t:
        check_stored_report(t["raw0"], u, Eacc, what + "raw0", "raw0", report)
        want = stem_pool_exact(t["raw0"], t["bn1.scale"], t["bn1.shift"])
        assert bool((want.float()[negative] < 0).all())                    # the exact form is negative there too: 0 from a padding would differ
        same = torch.equal(t["pool0"].contiguous().view(torch.int16), want.contiguous().view(torch.int16))
        assert same, what + "pool0 is not the pool kernel's formula on the stored raw0: %d elements differ" % int((t["pool0"].float() != want.float()).sum())
    # (the un-fused stem is inside the derived bound too: same rounding points)
    check_stored_report(t["pool0"], ref, E, what + "pool0", "pool0", report)
    return int(negative.sum())


def eval_check_block(t, i, g, x, report, what=""):
    """one bottleneck of the inference forward from its stored input x: a1, a2, then y by the path the plan took ("block<i>.wcat" in t: the
    folded GEMM; a downsample branch: rawd and the res_scale / bias output stage; else the identity).  g: tests/test_gpu_resnet_plan.geometry's
    entry.  -> the stored y"""
    b = "block%d." % i
    W, S, H = (lambda c: t[b + "conv%s.w" % c]), (lambda c: t[b + "bn%s.scale" % c]), (lambda c: t[b + "bn%s.shift" % c])
    ref, E = eval_conv_act(x, W("1"), 1, 0, S("1"), H("1"))
    check_stored_report(t[b + "a1"], ref, E, what + "a1", "a1", report)
    ref, E = eval_conv_act(t[b + "a1"], W("2"), g["stride"], 1, S("2"), H("2"))
    check_stored_report(t[b + "a2"], ref, E, what + "a2", "a2", report)
    if b + "wcat" in t:
        ref, E = eval_y_folded(t[b + "a2"], x, t[b + "wcat"], t[b + "shcat"])
        check_stored_report(t[b + "y"], ref, E, what + "y (folded)", "y folded", report)
    elif g["has_ds"]:
        ref, E = eval_conv(x, W("d"), g["stride"], 0)
        check_stored_report(t[b + "rawd"], ref, E, what + "rawd", "rawd", report)
        ref, E = eval_y(t[b + "a2"], W("3"), S("3"), H("3"), t[b + "rawd"], S("d"), H("d"))
        check_stored_report(t[b + "y"], ref, E, what + "y (branch)", "y branch", report)
    else:
        ref, E = eval_y(t[b + "a2"], W("3"), S("3"), H("3"), x)
        check_stored_report(t[b + "y"], ref, E, what + "y (identity)", "y identity", report)
    return t[b + "y"]


def eval_check_head(y, feat, emb, mode, neck, report, what=""):
    """feat from the last y in feature mode `mode`, the embedding from feat; neck = (weight, bias, running_mean, running_var)"""
    ref, bound = eval_feat(y, mode)
    if mode == "gmp":
        assert torch.equal(feat.double(), ref), what + "feat (gmp) is not the maximum"
    else:
        report["feat " + mode] = max(report.get("feat " + mode, 0.0), float(((feat.double() - ref).abs() / bound).max()))
        assert_within(feat.double(), ref, bound, what + "feat (%s)" % mode)
    check_neck_eval(emb, feat, neck[0], neck[1], neck[2], neck[3], what + "embedding (%s)" % mode)
