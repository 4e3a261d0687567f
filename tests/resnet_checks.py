"""Checks shared by tests/test_gpu_nnops_plan_sizes.py (the BatchNorm / pooling kernels on their own, exact operands) and
tests/test_gpu_resnet_plan.py (the same kernels as the ResNet plan launches them, on the plan's own tensors): one derivation, one bound.
The first part was moved here from test_gpu_nnops_plan_sizes.py unchanged; the second part restates the same derivations for general
(not power-of-two, not integer) operands, every extra rounding charged where it happens."""
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
