"""CPU: the numpy twin of the meta-recognition contract (tests/metarec_ref.py) against the reference's own libmr / Meta_Recognition
(tests/golden/metarec.npz, written by tests/golden/make_metarec_golden.py) at the bounds of tests/metarec_checks.py, and the behaviour
the contract adds on top of the reference."""
import numpy as np
import pytest

import metarec_ref as R
from conftest import load_golden
from metarec_checks import case, check_fit, check_fused, golden_cases


@pytest.fixture(scope="module")
def golden():
    return load_golden("metarec.npz")


def test_golden_has_the_cases(golden):
    metas = {tuple(int(v) for v in golden[n + "/meta"]) + (float(golden[n + "/killscale"]),) for n in golden_cases(golden)}
    assert metas == {(12, 33, 3, 0, 1, 1.0), (40, 33, 5, 0, 1, 1.0), (64, 40, 20, 0, 1, 1.0), (64, 40, 20, 1, 1, 1.0), (40, 33, 5, 0, 1, 0.5),
                     (72, 96, 20, 0, 3, 1.0)}


def test_twin_matches_reference(golden):
    for name in golden_cases(golden):
        c = case(golden, name)
        for a in range(c["m"]):
            fits, small, n_unfit = R.metarec(c["S"][a], c["topk"], c["use_columns"], c["killscale"])
            assert n_unfit == 0
            check_fit((fits, small, R.wscore(c["S"][a], fits, small)), (c["fits"][a], c["small"][a], c["w"][a]), "%s model %d" % (name, a))
        if c["fused"] is not None:
            fused, _ = R.mrfuse(c["S"], c["topk"], c["use_columns"], c["killscale"])
            check_fused(fused, c["fused"], sum(c["w"]), name)


def test_kill_order_and_transpose():
    S = np.array([[0.5, 0.25, 0.5, -1.0], [0.0, 0.125, 0.125, 0.125], [1.0, 2.0, 3.0, 4.0]], dtype=np.float32)
    KT = R.kill_transpose(S, 2)                                          # rows: the two largest, ties by ascending index
    assert np.array_equal(KT.T, np.array([[0, 0.25, 0, -1.0], [0, 0, 0, 0.125], [1, 2, 0, 0]], dtype=np.float32))
    KT = R.kill_transpose(S, 1, use_columns=True, killscale=0.5)
    assert np.array_equal(KT.T, np.array([[0.5, 0.25, 0.5, -1.0], [0, 0.125, 0.125, 0.125], [0.5, 1, 1.5, 2]], dtype=np.float32))
    assert KT.shape == (4, 3) and KT.dtype == np.float32


def test_tail_keeps_ties_above_the_boundary():
    row = np.array([0.5, 0.25, 0.5, 0.5, 0.125], dtype=np.float32)
    # T = 2: boundary key = the 4th smallest (0.5 at index 2); the tail is indices 2 and 3, both x = 1, so the row cannot be fitted
    shape, scale, small, _ = R.fit_row(row, 2)
    assert small == np.float32(0.5) and np.isnan(shape) and np.isnan(scale)


def test_constant_column_is_unfit_with_zero_weight():
    g = np.random.default_rng(0)
    S = g.uniform(0.1, 0.9, (30, 6)).astype(np.float32)
    S[:, 2] = 0.375
    fits, small, n_unfit = R.metarec(S, 3, use_columns=True)
    assert n_unfit == 1 and np.isnan(fits[2]).all() and np.isfinite(np.delete(fits, 2, 0)).all()
    w = R.wscore(S, fits, small)
    assert (w[:, 2] == 0).all() and (np.delete(w, 2, 1) > 0).any()


def test_tail_of_one_makes_every_row_unfit():
    g = np.random.default_rng(1)
    x = g.uniform(-1, 1, (5, 9)).astype(np.float32)
    fits, small, n_unfit, iters = R.fit_rows(x, 1)
    # one term: f = -1/k and f' = 1/k^2, so k doubles until the steps run out or exp(k L) overflows (x_t is 1 only up to rounding)
    assert n_unfit == 5 and np.isnan(fits).all() and (iters > 30).all() and (iters <= 100).all()
    assert np.array_equal(small, x.max(axis=1))
    assert (R.wscore(x.T[:4], fits, small) == 0).all()


def test_all_zero_weights_fall_back_to_the_mean():
    g = np.random.default_rng(2)
    S = [g.uniform(-1, 1, (4, 5)).astype(np.float32) for _ in range(3)]
    unfit = np.full((5, 2), np.nan)
    small = np.zeros(5, np.float32)
    fused, den = R.fuse_fitted(S, [unfit] * 3, [small] * 3)
    assert (den == 0).all()
    assert np.array_equal(fused, (S[0].astype(np.float64) + S[1] + S[2]) / 3)
    # one fitted model: where its w-score is 0 (d == 0) the mean, elsewhere that model's score alone
    fit = np.tile(np.array([2.0, 1.0]), (5, 1))
    small1 = np.full(5, 1.25, np.float32)                                 # d = max(s + 1 - 1.25, 0): 0 for s <= 0.25
    fused, den = R.fuse_fitted(S, [fit, unfit, unfit], [small1, small, small])
    zero = S[0] <= 0.25
    assert zero.any() and (~zero).any() and np.array_equal(den == 0, zero)
    assert np.array_equal(fused[zero], ((S[0].astype(np.float64) + S[1] + S[2]) / 3)[zero])
    np.testing.assert_allclose(fused[~zero], S[0].astype(np.float64)[~zero], rtol=1e-15)
