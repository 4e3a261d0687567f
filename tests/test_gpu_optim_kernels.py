"""GPU: dali_adam_step and dali_ema_update (csrc/optim.hip) through the C ABI on plain tensors, against the fp64 restatements of
tests/loss_kernels_ref.py, at sizes on both sides of the grid cap (2048 blocks x 1024 elements: beyond it a thread makes further grid-stride
passes) up to the flat parameter count of ResNet50ReID and past it."""
import numpy as np
import pytest
import torch

import loss_kernels_ref as R

pytestmark = pytest.mark.gpu

CAP = 2048 * 1024                                      # elements one pass of the capped grid covers
B1, B2, EPS = 0.9, 0.999, 1e-8


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from daliid_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def resnet_count(lib):
    from daliid_amd import Encoders
    n = int(Encoders.ResNet50ReID().flat_params.numel())
    torch.cuda.empty_cache()
    assert n % 4 == 0 and n > 8 * CAP
    return n


SIZES = ("n4", "n1020", "grid_cap", "grid_cap_plus4", "resnet50", "24Mi_plus1028")


def _size(which, resnet_count):
    return dict(zip(SIZES, (4, 1020, CAP, CAP + 4, resnet_count, 24 * 2 ** 20 + 1028)))[which]


def _adam(lib, p, g, m, v, n, lr, wd, step, gs, wsum, b1=B1, b2=B2, eps=EPS):
    """the raw status of dali_adam_step on the first n elements of the given tensors"""
    return lib.lib().dali_adam_step(lib.ctx(p.device), lib.stream_ptr(), lib.ptr(p), lib.ptr(g), lib.ptr(m), lib.ptr(v), n, lr, b1, b2, eps, wd, step,
                                    gs, lib.ptr(wsum))


def _ema(lib, mom, theta, n, beta):
    return lib.lib().dali_ema_update(lib.ctx(mom.device), lib.stream_ptr(), lib.ptr(mom), lib.ptr(theta), n, beta)


def _padding(n, rng):
    """a few runs of alignment padding (p = g = 0), as the flat parameter buffer has between tensors"""
    pad = np.zeros(n, bool)
    if n >= 1020:
        for s in rng.integers(0, n - 16, 8):
            pad[s:s + int(rng.integers(1, 16))] = True
        pad[-3:] = True
    if n > CAP:
        pad[CAP:CAP + 4] = False                       # the first elements of the second grid-stride pass stay live
    return pad


def _state(n, seed):
    rng = np.random.default_rng(seed)
    pad = _padding(n, rng)
    p = (rng.standard_normal(n, dtype=np.float32) * np.float32(0.02))
    p[pad] = 0
    return rng, pad, p


def _grad(n, rng, pad, scale):
    g = rng.standard_normal(n, dtype=np.float32) * np.float32(scale)
    g[pad] = 0
    return g


CALLS = ((1, 3.5e-4), (2, 3.5e-5), (1000, 1e-3))      # (step number, learning rate) of three consecutive calls


def _three_calls(lib, n, wd, gs, seed):
    """Every call is compared with the fp64 step from the state the GPU held before it, so each bound is the bound of one call."""
    rng, pad, p0 = _state(n, seed)
    assert n <= CAP or not pad[CAP:CAP + 4].any()
    p, m, v = (torch.from_numpy(a).cuda() for a in (p0, np.zeros(n, np.float32), np.zeros(n, np.float32)))
    wsum = torch.zeros(1, device="cuda")
    for step, lr in CALLS:
        g0 = _grad(n, rng, pad, 1e-2 / gs)
        before = [t.cpu().numpy() for t in (p, m, v)]
        g = torch.from_numpy(g0).cuda()
        assert _adam(lib, p, g, m, v, n, lr, wd, step, gs, wsum) == 0, lib.last_error()
        got_p, got_m, got_v = (t.cpu().numpy() for t in (p, m, v))
        assert np.array_equal(g.cpu().numpy(), g0)
        rp, rm, rv = R.adam_step(before[0], g0, before[1], before[2], lr, B1, B2, EPS, wd, step, gs)
        tm, tv = R.adam_moment_tols(before[0], g0, before[1], before[2], B1, B2, wd, gs)
        # tolerance of tests/test_gpu_losses.py::test_fused_adam_and_ema_match_torch
        np.testing.assert_allclose(got_p, rp, rtol=2e-6, atol=1e-8, err_msg="params n=%d step=%d" % (n, step))
        for name, got, ref, tol in (("exp_avg", got_m, rm, tm), ("exp_avg_sq", got_v, rv, tv)):
            err = np.abs(got.astype(np.float64) - ref)
            worst = int(np.argmax(err - tol))
            print("n=%d step=%d %s: max error / bound = %.3f" % (n, step, name, float(np.max(err / np.maximum(tol, 1e-300)))))
            assert np.all(err <= tol), "%s n=%d step=%d: element %d got %r, reference %r, bound %.3g" % (name, n, step, worst, got[worst],
                                                                                                           ref[worst], tol[worst])
        # the reduction alone: against the sum of the GPU's own updated parameters, at that test's rtol
        assert np.isclose(wsum.item(), float(np.square(got_p.astype(np.float64)).sum()), rtol=1e-5, atol=0), (n, step)
        for a in (got_p, got_m, got_v):
            assert not a[pad].any(), "padding (p = g = 0) must stay exactly 0"


@pytest.mark.parametrize("wd,gs", [(0.0, 1.0), (5e-4, 0.125)])
@pytest.mark.parametrize("which", SIZES)
def test_adam_three_calls_match_fp64(lib, resnet_count, which, wd, gs):
    _three_calls(lib, _size(which, resnet_count), wd, gs, seed=800 + SIZES.index(which))


def test_adam_subrange_leaves_the_rest_alone(lib):
    """FusedAdam launches on sub-ranges [b, e) of the flat buffers (the ViT's frozen tensors lie between them)."""
    N, b, e = CAP + 8192, 1028, CAP + 4100             # the range itself is longer than one pass of the grid
    rng, pad, p0 = _state(N, 900)
    g0, m0 = _grad(N, rng, pad, 1e-2), _grad(N, rng, pad, 1e-3)
    v0 = np.square(_grad(N, rng, pad, 1e-2))
    p, g, m, v = (torch.from_numpy(a).cuda() for a in (p0, g0, m0, v0))
    wsum = torch.zeros(1, device="cuda")
    assert _adam(lib, p[b:e], g[b:e], m[b:e], v[b:e], e - b, 3.5e-4, 5e-4, 7, 1.0, wsum) == 0, lib.last_error()
    rp, rm, rv = R.adam_step(p0[b:e], g0[b:e], m0[b:e], v0[b:e], 3.5e-4, B1, B2, EPS, 5e-4, 7, 1.0)
    np.testing.assert_allclose(p.cpu().numpy()[b:e], rp, rtol=2e-6, atol=1e-8)
    tm, tv = R.adam_moment_tols(p0[b:e], g0[b:e], m0[b:e], v0[b:e], B1, B2, 5e-4, 1.0)
    assert np.all(np.abs(m.cpu().numpy()[b:e] - rm) <= tm) and np.all(np.abs(v.cpu().numpy()[b:e] - rv) <= tv)
    for t, a in ((p, p0), (g, g0), (m, m0), (v, v0)):
        got = t.cpu().numpy()
        assert np.array_equal(got[:b].view(np.uint32), a[:b].view(np.uint32)) and np.array_equal(got[e:].view(np.uint32), a[e:].view(np.uint32))
    assert np.array_equal(g.cpu().numpy(), g0)
    assert np.isclose(wsum.item(), float(np.square(p.cpu().numpy()[b:e].astype(np.float64)).sum()), rtol=1e-5, atol=0)


@pytest.mark.parametrize("n", [1020, CAP + 4])
def test_adam_without_weight_sum_gives_the_same_parameters(lib, n):
    rng, pad, p0 = _state(n, 910)
    g0 = _grad(n, rng, pad, 1e-2)
    outs = []
    for wsum in (torch.zeros(1, device="cuda"), None):
        p, g, m, v = (torch.from_numpy(a).cuda() for a in (p0, g0, np.zeros(n, np.float32), np.zeros(n, np.float32)))
        assert _adam(lib, p, g, m, v, n, 3.5e-4, 5e-4, 1, 1.0, wsum) == 0, lib.last_error()
        outs.append([t.cpu().numpy() for t in (p, m, v)])
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert not np.array_equal(outs[0][0], p0)


def test_adam_refusals_change_nothing(lib):
    n = 1024
    rng, pad, p0 = _state(n + 4, 920)
    arrays = (p0, _grad(n + 4, rng, pad, 1e-2), _grad(n + 4, rng, pad, 1e-3), np.square(_grad(n + 4, rng, pad, 1e-2)))
    p, g, m, v = (torch.from_numpy(a).cuda() for a in arrays)
    wsum = torch.full((1,), -3.0, device="cuda")
    assert _adam(lib, p, g, m, v, 1022, 3.5e-4, 5e-4, 1, 1.0, wsum) != 0            # n % 4
    assert _adam(lib, p, g, m, v, 0, 3.5e-4, 5e-4, 1, 1.0, wsum) != 0               # n = 0
    assert _adam(lib, p, g, m, v, n, 3.5e-4, 5e-4, 0, 1.0, wsum) != 0               # step = 0
    for k in range(4):                                                               # each pointer in turn offset by 4 bytes
        args = [t[1:] if j == k else t for j, t in enumerate((p, g, m, v))]
        assert _adam(lib, *args, n, 3.5e-4, 5e-4, 1, 1.0, wsum) != 0
        assert "aligned" in lib.last_error()
    torch.cuda.synchronize()
    for t, a in zip((p, g, m, v), arrays):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), a.view(np.uint32))
    assert wsum.item() == -3.0
    assert _adam(lib, p, g, m, v, n, 3.5e-4, 5e-4, 1, 1.0, wsum) == 0, lib.last_error()   # and the same arguments, valid, are accepted


@pytest.mark.parametrize("which", SIZES)
def test_ema_matches_fp64(lib, resnet_count, which):
    n, guard = _size(which, resnet_count), 8
    rng = np.random.default_rng(950 + SIZES.index(which))
    # beta = 0.5 on integers below 2^20: every product and the sum are exact
    m0 = rng.integers(-2 ** 20, 2 ** 20, n + guard).astype(np.float32) * 2
    t0 = rng.integers(-2 ** 20, 2 ** 20, n + guard).astype(np.float32) * 2
    mom, theta = torch.from_numpy(m0).cuda(), torch.from_numpy(t0).cuda()
    assert _ema(lib, mom, theta, n, 0.5) == 0, lib.last_error()
    got = mom.cpu().numpy()
    assert np.array_equal(got[:n].astype(np.float64), R.ema(m0[:n], t0[:n], 0.5))
    assert np.array_equal(got[n:], m0[n:]) and np.array_equal(theta.cpu().numpy(), t0)
    # beta = 0.999, tolerance of tests/test_gpu_losses.py::test_fused_adam_and_ema_match_torch
    m0 = rng.standard_normal(n + guard, dtype=np.float32)
    t0 = rng.standard_normal(n + guard, dtype=np.float32)
    mom, theta = torch.from_numpy(m0).cuda(), torch.from_numpy(t0).cuda()
    assert _ema(lib, mom, theta, n, 0.999) == 0, lib.last_error()
    got = mom.cpu().numpy()
    np.testing.assert_allclose(got[:n], R.ema(m0[:n], t0[:n], 0.999), rtol=1e-6, atol=1e-9)
    assert np.array_equal(got[n:], m0[n:]) and np.array_equal(theta.cpu().numpy(), t0)


def test_ema_refusals_change_nothing(lib):
    n = 1024
    rng = np.random.default_rng(960)
    m0, t0 = rng.standard_normal(n + 4, dtype=np.float32), rng.standard_normal(n + 4, dtype=np.float32)
    mom, theta = torch.from_numpy(m0).cuda(), torch.from_numpy(t0).cuda()
    assert _ema(lib, mom, theta, 1022, 0.999) != 0
    assert _ema(lib, mom, theta, 0, 0.999) != 0
    assert _ema(lib, mom[1:], theta, n, 0.999) != 0
    assert _ema(lib, mom, theta[1:], n, 0.999) != 0
    torch.cuda.synchronize()
    assert np.array_equal(mom.cpu().numpy(), m0) and np.array_equal(theta.cpu().numpy(), t0)
