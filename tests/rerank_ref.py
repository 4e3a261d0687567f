"""numpy restatement of k-reciprocal re-ranking as include/daliid.h (dali_rerank) defines it; test infrastructure only.

V is kept sparse (scipy.sparse.csr_matrix, fp32), so N ~ 50k runs on a CPU.  For a case whose blocks live on a GPU the caller passes
the pieces that would need the dense matrix: ``colmax``, the neighbour lists ``R`` (first k1 + 1 columns of the stable argsort of C)
and ``full_at(rows, cols)``, a vectorised reader of full[rows, cols] = [[q_q, q_g], [q_g^T, g_g]][rows, cols].
"""
import numpy as np
import scipy.sparse as sp

F32 = np.float32


def half_k(k1):
    """h = np.around(k1 / 2): round half to even (k1 = 5 -> 2, k1 = 7 -> 4, k1 = 20 -> 10)."""
    return int(np.around(k1 / 2.0))


def full_matrix(q_g, q_q, g_g):
    return np.block([[q_q, q_g], [q_g.T, g_g]]).astype(F32)


def dense_C(q_g, q_q, g_g):
    """C = (A / max(A, axis=0))^T with A = full ** 2, in fp32."""
    A = full_matrix(q_g, q_q, g_g) ** 2
    return (A / A.max(axis=0)).T


def colmax_from_blocks(q_g, q_q, g_g):
    """max(A, axis=0) without building A: column i of A is column i of q_q over row i of q_g (queries), column i of q_g over
    column i of g_g (gallery)."""
    sq = lambda x: np.asarray(x, F32) ** 2
    return np.concatenate([np.maximum(sq(q_q).max(axis=0), sq(q_g).max(axis=1)),
                           np.maximum(sq(q_g).max(axis=0), sq(g_g).max(axis=0))]).astype(F32)


def neighbour_lists(C, K):
    return np.argsort(C, axis=1, kind="stable")[:, :K].astype(np.int64)


def reciprocal_sets(R, K, h):
    """-> (KR, KRh): lists of int arrays.  KR[i] = {f in R[i][:K] : i in R[f][:K]}, KRh the same with h + 1 neighbours."""
    N = R.shape[0]
    idx = np.arange(N)[:, None, None]
    fwd = R[:, :K]
    kr_mask = (R[fwd, :K] == idx).any(axis=2)
    fwd_h = R[:, :h + 1]
    krh_mask = (R[fwd_h, :h + 1] == idx).any(axis=2)
    return [fwd[i][kr_mask[i]] for i in range(N)], [fwd_h[i][krh_mask[i]] for i in range(N)]


def expansion_sets(KR, KRh):
    """E(i): sorted union of KR(i) and every KRh(c), c in KR(i), with |KRh(c) & KR(i)| > (2.0/3.0) * |KRh(c)| (double)."""
    E = []
    for i in range(len(KR)):
        kr = set(KR[i].tolist())
        e = set(kr)
        for c in KR[i].tolist():
            cand = KRh[c]
            inter = sum(1 for x in cand.tolist() if x in kr)
            if float(inter) > (2.0 / 3.0) * float(len(cand)):
                e.update(cand.tolist())
        E.append(np.array(sorted(e), dtype=np.int64))
    return E


def re_ranking_ref(q_g, q_q=None, g_g=None, k1=20, k2=6, lambda_value=0.3, R=None, colmax=None, full_at=None, return_parts=False):
    """-> out fp32 [nq, ng] (and, with return_parts, a dict of the intermediate sets and matrices)."""
    q_g = np.asarray(q_g, F32)
    nq, ng = q_g.shape
    N, K, h = nq + ng, k1 + 1, half_k(k1)
    assert 1 <= k1 and K <= N and 1 <= k2 <= K and 0.0 <= lambda_value <= 1.0
    if full_at is None:
        full = full_matrix(q_g, np.asarray(q_q, F32), np.asarray(g_g, F32))
        full_at = lambda rows, cols: full[rows, cols]
    if colmax is None:
        colmax = colmax_from_blocks(q_g, q_q, g_g)
    colmax = np.asarray(colmax, F32)
    if R is None:
        R = neighbour_lists(dense_C(q_g, q_q, g_g), K)
    R = np.asarray(R, np.int64)[:, :K]
    KR, KRh = reciprocal_sets(R, K, h)
    E = expansion_sets(KR, KRh)
    # V: w_e = exp(-C[i, e]) in fp32, C[i, e] = full[e, i]^2 / colmax[i]; the sum in fp64, rounded to fp32 once
    lens = np.array([len(e) for e in E], dtype=np.int64)
    rows = np.repeat(np.arange(N), lens)
    cols = np.concatenate(E) if N else np.zeros(0, np.int64)
    x = np.asarray(full_at(cols, rows), F32)
    w = np.exp(-((x * x) / colmax[rows])).astype(F32)
    indptr = np.concatenate([[0], np.cumsum(lens)])
    sums = np.array([np.float64(w[indptr[i]:indptr[i + 1]].astype(np.float64).sum()) for i in range(N)]).astype(F32)
    V = sp.csr_matrix(((w / sums[rows]).astype(F32), cols, indptr), shape=(N, N), dtype=F32)
    V1 = V
    if k2 != 1:                                   # mean of V[R[i][:k2]]: fp32 sums in R order, then / k2
        acc = V[R[:, 0]]
        for r in range(1, k2):
            acc = (acc + V[R[:, r]]).astype(F32)
        acc = sp.csr_matrix(acc, dtype=F32)
        acc.data = (acc.data / F32(k2)).astype(F32)
        V = acc
    V = sp.csr_matrix(V, dtype=F32)
    V.sort_indices()
    # Jaccard: per query, the columns of V[i] in ascending order, each adding min(V[i,c], V[j,c]) to t[j] (fp32)
    Vg = sp.csc_matrix(V[nq:], dtype=F32)
    Vg.sort_indices()
    Cq = ((q_g * q_g) / colmax[:nq, None]).astype(F32)
    out = np.empty((nq, ng), F32)
    for i in range(nq):
        t = np.zeros(ng, F32)
        lo, hi = V.indptr[i], V.indptr[i + 1]
        for c, v in zip(V.indices[lo:hi], V.data[lo:hi]):
            a, b = Vg.indptr[c], Vg.indptr[c + 1]
            g = Vg.indices[a:b]
            t[g] = t[g] + np.minimum(F32(v), Vg.data[a:b])
        jac = F32(1) - t / (F32(2) - t)
        out[i] = jac * F32(1.0 - lambda_value) + Cq[i] * F32(lambda_value)
    if return_parts:
        return out, dict(R=R, KR=KR, KRh=KRh, E=E, V1=V1, V=V, colmax=colmax, h=h)
    return out


def tie_gaps(C_sorted_rows, k1, k2):
    """Smallest gap between the sorted C values at the positions whose order decides a set: k1/k1+1 (0-based), h/h+1, k2-1/k2."""
    h = half_k(k1)
    s = np.asarray(C_sorted_rows, np.float64)
    pos = [p for p in {k1, h, k2 - 1} if p + 1 < s.shape[1]]
    return min(float((s[:, p + 1] - s[:, p]).min()) for p in pos)
