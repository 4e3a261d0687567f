"""GPU: the loss-head kernels of csrc/losses.hip, each fed a crafted fp32 similarity matrix (no GEMM between the input and the assertion) and
compared with the fp64 restatements of tests/loss_kernels_ref.py: selections exactly, everything else within the bounds derived there.  The
goldens (tests/test_gpu_losses.py) pin these heads to the reference's program end to end; this file pins what the goldens cannot reach: rows of
255..5120 proxies on both code paths of proxy_rows_kernel, ties, several centers per identity, and the backward arguments of the data-parallel
path (denom, gscale, accumulate)."""
import numpy as np
import pytest
import torch

import loss_kernels_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def L():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from daliid_amd import losses
    return losses


@pytest.fixture(scope="module")
def KMAX(L):
    return L._kmax()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def within(got, ref, tol, what):
    got, ref, tol = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(tol, np.float64)
    assert np.all(np.isfinite(got)), what + ": not finite"
    err = np.abs(got - ref)
    ratio = float(np.max(err / np.maximum(tol, 1e-300))) if err.size else 0.0
    print("%s: max error / bound = %.3f" % (what, ratio))
    bad = err > tol
    assert not bad.any(), "%s: %d outside the bound, worst error/bound %.3g at %s (got %r, reference %r)" % (
        what, int(bad.sum()), ratio, np.unravel_index(np.argmax(err / np.maximum(tol, 1e-300)), err.shape),
        got.flat[np.argmax(err / np.maximum(tol, 1e-300))], ref.flat[np.argmax(err / np.maximum(tol, 1e-300))])


# --------------------------------------------------------------------------------------------------------------------------------- proxy forward
@pytest.fixture(scope="module")
def proxy_inputs(KMAX):
    cases = R.proxy_cases(KMAX)
    assert tuple(sorted(cases)) == R.PROXY_CASE_NAMES
    return cases


def _run_proxy(L, S, y, pl, w, tau):
    rowstat, sums, sel_idx, sel_coef, status = L.proxy_fwd(dev(S), dev(y), dev(pl), dev(w), tau)
    return host(rowstat), host(sums), host(sel_idx), host(sel_coef), int(status.item())


@pytest.mark.parametrize("name", R.PROXY_CASE_NAMES)
def test_proxy_forward_matches_fp64(L, KMAX, proxy_inputs, name):
    S, y, pl, w, tau = proxy_inputs[name]
    ref = R.proxy_rows(S, y, pl, w, tau, KMAX)
    rowstat, sums, sel_idx, sel_coef, status = _run_proxy(L, S, y, pl, w, tau)
    assert status == ref["status"]
    ok = ref["specified"]                        # a row whose identity has more than KMAX proxies is unspecified
    assert torch.equal(torch.from_numpy(sel_idx[ok]), torch.from_numpy(ref["sel_idx"][ok])), \
        "selection differs in rows %s" % np.flatnonzero(ok & (sel_idx != ref["sel_idx"]).any(axis=1))[:8]
    within(sel_coef[ok], ref["sel_coef"][ok], ref["coef_tol"][ok], name + " sel_coef")
    within(rowstat[ok, 0], ref["num"][ok], ref["num_tol"][ok], name + " row numerator")
    assert np.array_equal(rowstat[ok, 1], ref["den"][ok].astype(np.float32))          # w, or exactly 0 for a row without a proxy
    none = ok & (ref["den"] == 0)
    assert np.all(sel_idx[none] == -1) and np.all(sel_coef[none] == 0) and np.all(rowstat[none] == 0)
    if ok.all():
        within(sums[0], ref["sums"][0], R.sums_tol(ref["num_tol"], ref["sums"][0]), name + " sum of numerators")
        within(sums[1], ref["sums"][1], R.sums_tol(0.0, ref["sums"][1]), name + " sum of weights")


@pytest.mark.parametrize("family", ["random", "ties"])
def test_proxy_register_and_long_row_paths_agree(L, proxy_inputs, family):
    """NP = 4096 is the longest row held in registers, 4097 the shortest that is re-read; the extra proxy is nobody's and the lowest."""
    a = _run_proxy(L, *proxy_inputs["np4096_" + family])
    b = _run_proxy(L, *proxy_inputs["np4097_" + family])
    assert np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3]) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# -------------------------------------------------------------------------------------------------------------------------------- proxy backward
@pytest.mark.parametrize("D", R.PROXY_BWD_DIMS)
def test_proxy_backward_exact_on_dyadic_inputs(L, KMAX, D):
    """Coefficients are multiples of 2^-4 up to 4, proxies integers up to 8, gscale and denom powers of two: every partial sum is a multiple of
    2^-4 below 2^11, exact in fp32 in any order, so the kernel must return the fp64 result bit for bit."""
    rng = np.random.default_rng(300 + D)
    nb, NPROX, guard = 37, 90, 3
    sel_idx, sel_coef = R.crafted_selection(nb, NPROX, KMAX, rng)
    P = rng.integers(-8, 9, (NPROX, D)).astype(np.float32)
    P[0] = 8.0                                                          # what an empty slot reads
    denom = np.array([64.0], np.float32)                                # not the local sum of anything
    ref = R.proxy_bwd(sel_idx, sel_coef, P, denom[0], gscale=0.25)
    got = L.proxy_bwd(dev(sel_idx), dev(sel_coef), dev(P), dev(denom), gscale=0.25)
    assert np.array_equal(host(got).astype(np.float64), ref)
    # accumulate into a buffer with guard rows behind it
    base = rng.integers(-16, 17, (nb + guard, D)).astype(np.float32)
    buf = dev(base)
    L.proxy_bwd(dev(sel_idx), dev(sel_coef), dev(P), dev(denom), gscale=0.25, out=buf, accumulate=True)
    ref = R.proxy_bwd(sel_idx, sel_coef, P, denom[0], gscale=0.25, accumulate=True, out=base[:nb])
    assert np.array_equal(host(buf)[:nb].astype(np.float64), ref)
    assert np.array_equal(host(buf)[nb:], base[nb:])
    # overwrite (accumulate = 0) ignores what the buffer held
    buf = dev(base)
    L.proxy_bwd(dev(sel_idx), dev(sel_coef), dev(P), dev(denom), gscale=0.25, out=buf, accumulate=False)
    assert np.array_equal(host(buf)[:nb].astype(np.float64), R.proxy_bwd(sel_idx, sel_coef, P, denom[0], gscale=0.25))
    assert np.array_equal(host(buf)[nb:], base[nb:])


@pytest.mark.parametrize("D", R.PROXY_BWD_DIMS)
def test_proxy_backward_random_within_bound(L, KMAX, D):
    sel_idx, sel_coef, P, denom, gscale, base = R.proxy_bwd_random_inputs(D, KMAX)
    denom = np.array([denom], np.float32)
    for acc in (False, True):
        buf = dev(base)
        L.proxy_bwd(dev(sel_idx), dev(sel_coef), dev(P), dev(denom), gscale=gscale, out=buf, accumulate=acc)
        ref = R.proxy_bwd(sel_idx, sel_coef, P, denom[0], gscale, acc, base)
        within(host(buf), ref, R.proxy_bwd_tol(sel_idx, sel_coef, P, denom[0], gscale, acc, base), "proxy_bwd D=%d accumulate=%d" % (D, acc))


# ------------------------------------------------------------------------------------------------------------------------------------ center head
@pytest.fixture(scope="module")
def center_inputs():
    cases = R.center_cases()
    assert tuple(sorted(cases)) == R.CENTER_CASE_NAMES
    return cases


@pytest.mark.parametrize("name", R.CENTER_CASE_NAMES)
def test_center_forward_and_backward_match_fp64(L, center_inputs, name):
    S, y, cl, w, tau, first = center_inputs[name]
    nb, NC = S.shape
    ref = R.center_rows(S, y, cl, w, tau)
    if first is not None:
        assert np.array_equal(ref["argmax"], first)                     # the crafted tie resolves to its lower column
    rowstat, sums = L.center_fwd(dev(S), dev(y), dev(cl), dev(w), tau)
    rowstat, sums = host(rowstat), host(sums)
    # in every row the two largest entries are equal, or too far apart for their products with 1/tau to coincide: the arg-max is exact
    assert R.top_two_separated(S).all()
    assert np.array_equal(rowstat[:, 2], ref["argmax"].astype(np.float32)), "arg-max differs"
    within(rowstat[:, 0], ref["num"], R.center_num_tol(ref, w, NC), name + " row numerator")
    assert np.array_equal(rowstat[:, 1], (w.astype(np.float64) * ref["cnt"]).astype(np.float32))      # w * cnt: one exact-input product
    within(rowstat[:, 3], ref["maxp"], R.center_maxp_tol(ref, NC), name + " max probability")
    within(sums[0], ref["sums"][0], R.sums_tol(R.center_num_tol(ref, w, NC), ref["sums"][0]), name + " sum of numerators")
    within(sums[1], ref["sums"][1], R.sums_tol(R.U * ref["den"], ref["sums"][1]), name + " sum of denominators")
    # backward: the local denominator, then a global one that differs from it and a gradient scale
    for denom, gscale in ((float(sums[1]), 1.0), (float(np.float32(2.75) * sums[1]), 0.25)):
        dn = np.array([denom], np.float32)
        dS = host(L.center_bwd(dev(S), dev(y), dev(cl), dev(w), tau, dev(dn), gscale=gscale))
        tol = R.center_bwd_tol(S, y, cl, w, tau, dn[0], gscale)
        within(dS, R.center_bwd(S, y, cl, w, tau, dn[0], gscale), tol, "%s dS denom=%g gscale=%g" % (name, denom, gscale))
        # each row of dS sums to coef * (cnt - cnt) = 0
        within(dS.astype(np.float64).sum(axis=1), np.zeros(nb), tol.sum(axis=1), name + " row sums of dS")


# ----------------------------------------------------------------------------------------------------------------------------------- triplet head
@pytest.mark.parametrize("nb", [6, 61, 64, 256])
@pytest.mark.parametrize("family,tau", [("ties", 0.05), ("random", 0.1)])
def test_triplet_forward_matches_fp64(L, nb, family, tau):
    S, y, w = R.triplet_inputs(nb, family, 500 + nb)
    ref = R.triplet_rows(S, y, w, tau)
    assert ref["sel_idx"][0, 0] == 0                                    # row 0's only same-identity sample is itself
    rowstat, sums, sel_idx, sel_coef, status = L.triplet_fwd(dev(S), dev(y), dev(w), tau)
    assert int(status.item()) == 0 == ref["status"]
    assert torch.equal(sel_idx.cpu(), torch.from_numpy(ref["sel_idx"]))
    within(host(sel_coef), ref["sel_coef"], ref["coef_tol"], "triplet coefficients")
    within(host(rowstat)[:, 0], ref["num"], ref["num_tol"], "triplet row terms")
    assert np.array_equal(host(rowstat)[:, 1], w)
    within(host(sums)[0], ref["sums"][0], R.sums_tol(ref["num_tol"], ref["sums"][0]), "triplet sum")
    within(host(sums)[1], ref["sums"][1], R.sums_tol(0.0, ref["sums"][1]), "triplet weight sum")


def test_triplet_forward_row_without_negative(L):
    y = np.full(6, 7, np.int32)
    S, _, w = R.triplet_inputs(6, "random", 9)
    ref = R.triplet_rows(S, y, w, 0.1)
    rowstat, sums, sel_idx, sel_coef, status = L.triplet_fwd(dev(S), dev(y), dev(w), 0.1)
    assert int(status.item()) == 1 == ref["status"]
    assert np.all(host(sel_idx) == -1) and np.all(host(sel_coef) == 0) and np.all(host(rowstat) == 0) and np.all(host(sums) == 0)


@pytest.mark.parametrize("nb", [6, 61, 64, 256])
def test_triplet_backward_exact_on_dyadic_inputs(L, nb):
    """Crafted selections: mutual picks (0 picks 1 as negative, 1 picks 0), a self-positive on the diagonal (-2c), a skipped row (-1, -1);
    coefficients multiples of 2^-4, gscale / denom a power of two: at most four such terms per element, exact."""
    rng = np.random.default_rng(600 + nb)
    sel_idx = np.stack([rng.integers(0, nb, nb), rng.integers(0, nb, nb)], axis=1).astype(np.int32)
    sel_coef = (rng.integers(1, 65, nb) / 16.0).astype(np.float32)
    sel_idx[0] = (0, 1)                  # self-positive; negative 1
    sel_idx[1] = (2, 0)                  # negative 0: mutual with row 0
    sel_idx[2] = (1, 0)                  # positive 1 while row 1's positive is 2: mutual positives
    sel_idx[3] = (-1, -1)
    sel_coef[3] = 0.0
    denom = np.array([32.0], np.float32)
    ref = R.triplet_bwd(sel_idx, sel_coef, denom[0], gscale=0.5)
    assert ref[0, 0] == -2.0 * sel_coef[0] * 0.5 / 32.0
    got = host(L.triplet_bwd(dev(sel_idx), dev(sel_coef), dev(denom), gscale=0.5))
    assert np.array_equal(got.astype(np.float64), ref)
    assert np.array_equal(got, got.T)


# ------------------------------------------------------------------------------------------------------------------------------ row-stat reduction
@pytest.mark.parametrize("nb", [1, 255, 257, 1031])
def test_rowstat_reduction_exact(L, nb):
    """rowstat_reduce_kernel through both strides it is launched with.  Integer weights below 2^12 make the denominators integers whose sum
    stays below 2^24: the fp32 result must be that integer.  The numerators (w ln 2 in the triplet head at S = 0, w 2 ln 4 in the center head)
    lie in [2^-1, 2^14), so they are multiples of 2^-24 and any partial sum of them fits in 53 bits: a sum in double is exact in every
    order, and the kernel must return its fp32 rounding."""
    rng = np.random.default_rng(700 + nb)
    w = rng.integers(1, 4096, nb).astype(np.float32)
    y = (np.arange(nb) % 2).astype(np.int32)
    rowstat, sums, sel_idx, sel_coef, status = L.triplet_fwd(dev(np.zeros((nb, nb), np.float32)), dev(y), dev(w), 0.1)
    rowstat, sums = host(rowstat), host(sums)
    assert int(status.item()) == (1 if nb == 1 else 0)                  # a single row has no negative and contributes (0, 0)
    if nb > 1:
        assert np.array_equal(rowstat[:, 1], w)
    assert float(sums[1]) == float(rowstat[:, 1].astype(np.float64).sum()) == (0.0 if nb == 1 else float(w.astype(np.float64).sum()))
    assert float(sums[0]) == float(np.float32(rowstat[:, 0].astype(np.float64).sum()))
    # center head (stride 4): every identity has two centers
    cl = np.array([0, 0, 1, 1], np.int32)
    rowstat, sums = L.center_fwd(dev(np.zeros((nb, 4), np.float32)), dev(y), dev(cl), dev(w), 0.1)
    rowstat, sums = host(rowstat), host(sums)
    assert np.array_equal(rowstat[:, 1], 2.0 * w)
    assert float(sums[1]) == 2.0 * float(w.astype(np.float64).sum())
    assert float(sums[0]) == float(np.float32(rowstat[:, 0].astype(np.float64).sum()))
    assert np.all(rowstat[:, 0] > 0)
