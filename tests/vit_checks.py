"""Checks shared by tests/test_gpu_nnops_plan_sizes.py (the LayerNorm kernel on its own) and tests/test_gpu_vit_plan.py (the same kernel as the ViT
plan launches it, on the plan's own tensors): one derivation, one bound."""
import numpy as np
import torch

U = 2.0 ** -24                      # fp32 unit roundoff
HB = 2.0 ** -8                      # bf16 unit roundoff (half an ulp, relative)


def ulp32(a):
    """fp32 ulp of |a| (float64 numpy in and out)"""
    return np.spacing(np.abs(np.asarray(a, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def assert_within(got, ref, bound, what):
    err = (got - ref).abs()
    bad = ~(err <= bound)                                        # NaN counts as bad
    if bad.any():
        i = int(torch.argmax(torch.where(bad, err - bound, torch.zeros_like(err)).flatten().nan_to_num(nan=1e300)))
        raise AssertionError("%s: %d elements off; worst at %d: got %r, ref %r, bound %r" % (
            what, int(bad.sum()), i, float(got.flatten()[i]), float(ref.flatten()[i]), float(bound.flatten()[i])))


def check_layernorm_fwd(y, mean, rstd, x, gamma, beta, eps, what="LayerNorm", y_bf16=True):
    """layernorm_fwd_kernel against fp64 on the same x (host tensors; y, mean, rstd from the kernel).
    mean: a per-lane sequential sum (<= 16 terms) and a 6-level butterfly, then / C: <= 24u sum|x| / C + 1 ulp;  rstd: the same
    sums of squares of (x - mean) + eps, sqrtf and the reciprocal: <= 32u relative;  y = (x - mean) * rstd * gamma + beta in fp32
    then bf16: one bf16 rounding plus the propagated mean / rstd errors and 4u of the terms.  y_bf16=False: the fp32 output (the plan's
    final norm), the same bound without the bf16 rounding."""
    xd = x.double()
    m64 = xd.mean(1)
    r64 = 1.0 / torch.sqrt(((xd - m64.unsqueeze(1)) ** 2).mean(1) + eps)
    dmu = 24 * U * xd.abs().mean(1) + torch.from_numpy(ulp32(m64.numpy()))
    assert_within(mean.double(), m64, dmu, what + " mean")
    assert_within(rstd.double(), r64, 32 * U * r64, what + " rstd")
    xh = (xd - m64.unsqueeze(1)) * r64.unsqueeze(1)
    ref = xh * gamma.double() + beta.double()
    E = gamma.double().abs() * (36 * U * xh.abs() + r64.unsqueeze(1) * dmu.unsqueeze(1)) + 4 * U * (beta.double().abs() + ref.abs())
    assert_within(y.double(), ref, HB * ref.abs() + (1 + HB) * E if y_bf16 else E, what + " y")


def check_bn1d_bwd(dx, dg, db, x, dy, gamma, mk, ik, what="bn1d"):
    """bn1d_bwd_kernel against fp64, from the kernel's own mean mk / invstd ik (float64); host tensors; db None = the launch without dbeta"""
    N = x.shape[0]
    xd, dyd = x.double(), dy.double()
    xh = (xd - mk) * ik
    s1, s2 = dyd.sum(0), (dyd * xh).sum(0)
    a2 = (dyd * xh).abs().sum(0)                                  # the kernel's xhat is fp32((fp32(x - mean)) * invstd): 2u each
    if db is not None:
        assert_within(db.double(), s1, torch.from_numpy(ulp32(s1.numpy())) + 2.0 ** -45 * dyd.abs().sum(0), what + " dbeta")
    assert_within(dg.double(), s2, torch.from_numpy(ulp32(s2.numpy())) + 2 * U * a2, what + " dgamma")
    # dx = sc*(dy - a - xh*b): <= 8u |sc|(|dy| + |a| + |xh b|), plus the kernel's b = s2/N off by <= 2u * sum|dy xh| / N
    sc = gamma.double() * ik
    ref = sc * (dyd - s1 / N - xh * (s2 / N))
    bound = sc.abs() * (8 * U * (dyd.abs() + (s1 / N).abs() + (xh * (s2 / N)).abs()) + xh.abs() * 2 * U * a2 / N)
    assert_within(dx.double(), ref, bound, what + " dx")
