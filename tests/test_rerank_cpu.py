"""CPU: the numpy restatement of k-reciprocal re-ranking (tests/rerank_ref.py) that the GPU kernel is checked against.  torchreid is not
available, so the restatement is pinned here by an independent dense writing, a hand-worked case and the definition's corner rules."""
import numpy as np
import pytest

import rerank_ref as RR

F32 = np.float32


def _dense_rerank(q_g, q_q, g_g, k1, k2, lam):
    """A second, dense writing of the definition (torchreid-style loops, dense V, np.minimum broadcast for the Jaccard)."""
    nq = q_g.shape[0]
    full = np.concatenate([np.concatenate([q_q, q_g], axis=1), np.concatenate([q_g.T, g_g], axis=1)], axis=0).astype(F32)
    A = np.power(full, 2).astype(F32)
    C = np.transpose(A / np.max(A, axis=0))
    N = C.shape[0]
    V = np.zeros_like(C)
    rank = np.argsort(C, kind="stable").astype(np.int32)
    h = int(np.around(k1 / 2.))
    for i in range(N):
        fwd = rank[i, :k1 + 1]
        bwd = rank[fwd, :k1 + 1]
        kr = fwd[np.where(bwd == i)[0]]
        exp = kr
        for c in kr:
            cf = rank[c, :h + 1]
            cb = rank[cf, :h + 1]
            ckr = cf[np.where(cb == c)[0]]
            if len(np.intersect1d(ckr, kr)) > 2. / 3 * len(ckr):
                exp = np.append(exp, ckr)
        exp = np.unique(exp)
        w = np.exp(-C[i, exp])
        V[i, exp] = w / F32(np.sum(w, dtype=np.float64))
    if k2 != 1:
        Vq = np.zeros_like(V)
        for i in range(N):
            Vq[i] = np.mean(V[rank[i, :k2], :], axis=0)
        V = Vq
    t = np.minimum(V[:nq, None, :], V[None, nq:, :]).sum(axis=2, dtype=F32)
    jac = F32(1) - t / (F32(2) - t)
    return jac * F32(1 - lam) + C[:nq, nq:] * F32(lam)


def _feature_blocks(nq, ng, d, seed, n_ids=None, noise=0.8, asym=0.0):
    rng = np.random.default_rng(seed)
    n_ids = n_ids or max(2, (nq + ng) // 6)
    centers = rng.standard_normal((n_ids, d))
    ids = rng.integers(0, n_ids, nq + ng)
    x = centers[ids] + noise * rng.standard_normal((nq + ng, d))
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    D = (1.0 - x @ x.T).astype(F32)
    if asym:                                      # the GPU distance kernel's blocks need not be bitwise symmetric
        D = (D + asym * rng.standard_normal(D.shape)).astype(F32)
    return D[:nq, nq:].copy(), D[:nq, :nq].copy(), D[nq:, nq:].copy()


@pytest.mark.parametrize("nq,ng,k1,k2,lam,seed", [
    (5, 40, 20, 6, 0.3, 0), (1, 30, 20, 6, 0.3, 1), (20, 120, 5, 6, 0.3, 2), (37, 250, 20, 1, 0.3, 3),
    (10, 90, 7, 3, 0.0, 4), (30, 270, 12, 13, 0.7, 5), (8, 60, 20, 21, 1.0, 6), (3, 4, 2, 1, 0.3, 7),
])
def test_sparse_restatement_matches_dense_writing(nq, ng, k1, k2, lam, seed):
    q_g, q_q, g_g = _feature_blocks(nq, ng, 16, seed, asym=1e-3 if seed % 2 else 0.0)
    ref = RR.re_ranking_ref(q_g, q_q, g_g, k1, k2, lam)
    dense = _dense_rerank(q_g, q_q, g_g, k1, k2, lam)
    assert ref.dtype == np.float32 and ref.shape == (nq, ng)
    np.testing.assert_allclose(ref, dense, rtol=0, atol=1e-6)


def test_hand_worked_two_clusters():
    """Six points, two tight clusters: A = {0, 2, 3}, B = {1, 4, 5}; queries 0 (A) and 1 (B), gallery 2, 3 (A), 4, 5 (B).
    Inside a cluster d(x, first mate) = 0.1, d(x, second) = 0.2 or 0.15 as listed below; across clusters d = 1."""
    D = np.ones((6, 6))
    np.fill_diagonal(D, 0.0)
    for a, b, v in [(0, 2, 0.1), (0, 3, 0.2), (2, 3, 0.15), (1, 4, 0.1), (1, 5, 0.2), (4, 5, 0.15)]:
        D[a, b] = D[b, a] = v
    D = D.astype(F32)
    nq, k1, k2, lam = 2, 2, 1, 0.3
    q_g, q_q, g_g = D[:nq, nq:], D[:nq, :nq], D[nq:, nq:]
    out, parts = RR.re_ranking_ref(q_g, q_q, g_g, k1, k2, lam, return_parts=True)
    # every column's max of D^2 is 1, so C = D^2; the three nearest of each point are its own cluster
    assert parts["h"] == 1
    assert parts["R"].tolist() == [[0, 2, 3], [1, 4, 5], [2, 0, 3], [3, 2, 0], [4, 1, 5], [5, 4, 1]]
    assert [sorted(s.tolist()) for s in parts["KR"]] == [[0, 2, 3], [1, 4, 5], [0, 2, 3], [0, 2, 3], [1, 4, 5], [1, 4, 5]]
    # with 2 neighbours: 3 and 5 are nobody's first mate
    assert [sorted(s.tolist()) for s in parts["KRh"]] == [[0, 2], [1, 4], [0, 2], [3], [1, 4], [5]]
    # every candidate's KRh lies inside KR (2/2 > 4/3, 1/1 > 2/3): E = the cluster
    assert [s.tolist() for s in parts["E"]] == [[0, 2, 3], [1, 4, 5], [0, 2, 3], [0, 2, 3], [1, 4, 5], [1, 4, 5]]
    # V rows over (first point, mate at 0.1, mate at the other distance): exp(-C) normalised
    def vrow(c):
        w = np.exp(-np.asarray(c, np.float64))
        return w / w.sum()
    v0, v2, v3 = vrow([0, 0.01, 0.04]), vrow([0.01, 0, 0.0225]), vrow([0.04, 0.0225, 0])       # over columns 0, 2, 3
    np.testing.assert_allclose(parts["V"].toarray()[0, [0, 2, 3]], v0, atol=1e-7)
    np.testing.assert_allclose(parts["V"].toarray()[2, [0, 2, 3]], v2, atol=1e-7)
    blend = lambda t, c: (1 - t / (2 - t)) * (1 - lam) + c * lam
    near = blend(np.minimum(v0, v2).sum(), 0.01)          # query and gallery at 0.1
    far = blend(np.minimum(v0, v3).sum(), 0.04)           # at 0.2
    # query 1 sees B exactly as query 0 sees A (same distances); across clusters t = 0 and C = 1 -> 0.7 + 0.3 = 1
    expect = np.array([[near, far, 1.0, 1.0], [1.0, 1.0, near, far]])
    np.testing.assert_allclose(out, expect, rtol=0, atol=1e-6)
    assert 0 < near < far < 1


@pytest.mark.parametrize("k1,h", [(1, 0), (2, 1), (3, 2), (5, 2), (7, 4), (9, 4), (20, 10), (21, 10), (63, 32)])
def test_half_k_rounds_half_to_even(k1, h):
    assert RR.half_k(k1) == h


def test_transposed_normalisation_on_asymmetric_input():
    """C = (A / max(A, axis=0))^T: row i of C is column i of A over that column's max.  With lambda = 1 the output is exactly
    C[:nq, nq:] = q_g^2 / colmax[:nq], where a query's column of A runs down q_q's column and along q_g's row."""
    rng = np.random.default_rng(11)
    nq, ng = 6, 14
    q_q = rng.uniform(0.1, 1.0, (nq, nq)).astype(F32)
    q_q[:, 0] = 0.2
    q_q[3, 0] = 3.0                                 # column 0's max is far above row 0's
    q_g = rng.uniform(0.1, 1.0, (nq, ng)).astype(F32)
    g = rng.uniform(0.1, 1.0, (ng, ng)).astype(F32)
    out = RR.re_ranking_ref(q_g, q_q, g, 5, 2, 1.0)
    A = RR.full_matrix(q_g, q_q, g) ** 2
    assert not np.array_equal(A, A.T)
    C = (A / A.max(axis=0)).T
    assert np.array_equal(out, C[:nq, nq:])
    assert np.array_equal(out[0], (q_g[0] ** 2 / F32(9.0)).astype(F32))                   # colmax[0] = 3^2, from q_q's column
    assert not np.allclose(out, ((A / A.max(axis=1)[:, None])[:nq, nq:]))                 # the untransposed reading differs


def test_lambda_one_is_the_normalised_block():
    q_g, q_q, g_g = _feature_blocks(9, 50, 8, 21)
    out = RR.re_ranking_ref(q_g, q_q, g_g, 20, 6, 1.0)
    assert np.array_equal(out, RR.dense_C(q_g, q_q, g_g)[:9, 9:])
