"""CPU: the references of tests/qe_ref.py pinned by hand-worked numbers and by each other (no GPU)."""
import numpy as np
import pytest

import qe_ref as R

F32 = np.float32

# 3 rows, d = 2, k = 2: every product and sum below is exact in fp32 (and 1 / k = 0.5), so the expected values are exact
POOL = np.array([[1, 2], [3, -4], [0.5, 8]], dtype=F32)
IDX = np.array([[0, 1], [1, 2], [2, 0]], dtype=np.int32)
SIM = np.array([[1.0, 0.5], [0.5, -0.5], [2.0, 0.25]], dtype=F32)
HAND = {
    0: [[2, -1], [1.75, 2], [0.75, 5]],                                     # plain means
    1: [[1.25, 0], [0.625, -3], [0.625, 8.25]],                             # (1*[1,2] + .5*[3,-4]) / 2, ...
    3: [[0.6875, 0.75], [0.15625, -0.75], [2.0078125, 32.015625]],          # weights 1, .125 | .125, -.125 (sign kept) | 8, .015625
}


@pytest.mark.parametrize("alpha", [0, 1, 3])
def test_combine_hand_worked(alpha):
    want = np.array(HAND[alpha], dtype=F32)
    assert np.array_equal(R.combine_f32(POOL, IDX, SIM, alpha, False), want)
    assert np.array_equal(R.combine_f32(POOL, IDX, (F32(1) - SIM).astype(F32), alpha, True), want)      # 1 - (1 - s) is exact here


def _random_case(rng, n, n_pool, d, k):
    pool = (rng.standard_normal((n_pool, d)) * rng.uniform(0.5, 2, (n_pool, 1))).astype(F32)
    idx = rng.integers(0, n_pool, (n, k)).astype(np.int32)
    val = rng.uniform(-1, 1, (n, k)).astype(F32)
    return pool, idx, val


@pytest.mark.parametrize("alpha", [0, 1, 2, 3, 16])
@pytest.mark.parametrize("k", [1, 10, 128])
def test_combine_f32_against_float64(alpha, k):
    """k products (one rounding each), k additions and the final scaling (reciprocal + product): at most (k + 2) roundings of 2^-24
    relative on a quantity bounded by sum_j |w_j x_j| / k, for fp32 weights taken as given."""
    rng = np.random.default_rng(100 * alpha + k)
    pool, idx, val = _random_case(rng, 9, 40, 7, k)
    got = R.combine_f32(pool, idx, val, alpha, False)
    w = np.ones_like(val) if alpha == 0 else val.copy()      # the fp32 weights as the kernel forms them: s, then alpha - 1 products
    for _ in range(alpha - 1):
        w = (w * val).astype(F32)
    terms = w.astype(np.float64)[:, :, None] * pool.astype(np.float64)[idx]
    want = terms.sum(axis=1) / k
    bound = (k + 2) * 2.0 ** -24 * np.abs(terms).sum(axis=1) / k
    assert np.all(np.abs(got.astype(np.float64) - want) <= bound)


def test_alpha_zero_is_the_plain_mean():
    rng = np.random.default_rng(5)
    pool, idx, val = _random_case(rng, 6, 11, 5, 4)
    got = R.combine_f32(pool, idx, val, 0, False)
    acc = np.zeros((6, 5), dtype=F32)
    for j in range(4):
        acc = (acc + pool[idx[:, j]]).astype(F32)
    assert np.array_equal(got, (acc * F32(0.25)).astype(F32))
    assert np.array_equal(got, R.combine_f32(pool, idx, val, 0, True))            # the values play no part


def test_combine_skips_indices_outside_the_pool():
    idx = np.array([[0, 7], [-1, 2], [2, 0]], dtype=np.int32)
    got = R.combine_f32(POOL, idx, SIM, 1, False)
    assert np.array_equal(got, np.array([[0.5, 1], [-0.125, -2], [0.625, 8.25]], dtype=F32))


def test_aqe_f64_one_iteration_by_hand():
    """two tight pairs: with k = 2 every row averages itself (sim 1) and its partner"""
    q = np.array([[2.0, 0.0]])
    g = np.array([[1.0, 0.1], [0.0, 3.0], [0.2, 1.0]])
    q1, g1, info = R.aqe_f64(q, g, 2, 3, 1, "all")
    c = 1.0 / np.hypot(1.0, 0.1)                           # cos(q0, g0)
    assert np.allclose(q1[0], (q[0] + c ** 3 * g[0]) / 2, rtol=1e-14)
    assert np.allclose(g1[0], (g[0] + c ** 3 * q[0]) / 2, rtol=1e-14)
    assert info[0]["gap"].shape == (4,) and np.all(info[0]["gap"] > 0) and np.allclose(info[0]["smin"][:2], c)
    q2, g2, _ = R.aqe_f64(q, g, 2, 3, 1, "gallery")
    assert q2 is not None and np.array_equal(q2, q) and g2.shape == g.shape
    c12 = (0.0 * 0.2 + 3.0 * 1.0) / (3.0 * np.hypot(0.2, 1.0))
    assert np.allclose(g2[1], (g[1] + c12 ** 3 * g[2]) / 2, rtol=1e-14)


def test_inp_f64_hand_worked():
    gp = np.array([1, 1, 2, 2, 3, 1]); gc = np.array([0, 1, 0, 1, 0, 1])
    qp = np.array([1, 2, 9, 3]); qc = np.array([0, 1, 0, 0])
    d = np.array([[0.1, 0.5, 0.2, 0.3, 0.4, 0.6],      # junk g0; kept order g2 g3 g4 g1 g5: matches at 3 and 4 -> 2 / 5
                  [0.3, 0.3, 0.1, 0.0, 0.2, 0.3],      # junk g3 (the nearest); kept order g2 g4 g0 g1 g5 (ties by index): match at 0 -> 1
                  [0.1, 0.2, 0.3, 0.4, 0.5, 0.6],      # identity 9 is not in the gallery: excluded
                  [0.1, 0.2, 0.3, 0.4, 0.0, 0.6]],     # identity 3 only at g4, same camera (junk): excluded
                 dtype=F32)
    minp, inp, last_rank, n_rel = R.inp_f64(d, qp, gp, qc, gc)
    assert n_rel.tolist() == [2, 1, 0, 0] and last_rank.tolist() == [4, 0, -1, -1]
    assert inp.tolist() == [0.4, 1.0, 0.0, 0.0] and minp == pytest.approx(0.7, rel=1e-15)
