"""numpy references of query expansion and mINP (no GPU):
  * combine_f32   the float32 emulation of dali_qe_combine's arithmetic order (include/daliid.h), bit for bit
  * aqe_f64       average / alpha-weighted query expansion and database augmentation restated in float64 from the description:
                  normalise, similarity to the whole pool (self included), the k most similar rows (stable order: ties by ascending
                  index), mean of feat[top] * sim[top] ** alpha over the UN-normalised rows; repeated ``times`` times
  * inp_f64       inverse negative penalty per query under the market1501 protocol with the project's (distance, index) order
"""
import numpy as np

F32 = np.float32


def combine_f32(pool, idx, val, alpha, val_is_distance):
    """out[i][c] = (sum_j w_ij * pool[idx[i][j]][c]) * (1 / k), every operation a float32 operation in the header's order.  Indices
    outside the pool are skipped (the kernel's behaviour; the wrapper then raises)."""
    pool = np.ascontiguousarray(pool, dtype=F32)
    idx = np.asarray(idx)
    val = np.asarray(val, dtype=F32)
    n, k = idx.shape
    s = (F32(1.0) - val).astype(F32) if val_is_distance else val
    if alpha == 0:
        w = np.ones_like(s)
    else:
        w = s.copy()
        for _ in range(alpha - 1):
            w = (w * s).astype(F32)
    acc = np.zeros((n, pool.shape[1]), dtype=F32)
    for j in range(k):
        g = idx[:, j]
        ok = (g >= 0) & (g < pool.shape[0])
        term = (w[:, j, None] * pool[np.where(ok, g, 0)]).astype(F32)
        acc = np.where(ok[:, None], (acc + term).astype(F32), acc)
    rk = F32(1.0) / F32(k)
    return (acc * rk).astype(F32)


def aqe_f64(q, g, k, alpha, times, expand):
    """-> (q', g', info) in float64.  info: one dict per iteration with, per expanded row, ``gap`` = sim[k-1] - sim[k] of the descending
    similarities (inf when k is the pool size), ``smin`` = the smallest top-k similarity, and ``scale`` = (1 / k) sum_j |w_j| |x_j|_2."""
    q = np.asarray(q, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    feat = np.concatenate([q, g]) if expand == "all" else g.copy()
    k = min(k, feat.shape[0])
    info = []
    for _ in range(times):
        unit = feat / np.linalg.norm(feat, axis=1, keepdims=True)
        sim = unit @ unit.T
        order = np.argsort(-sim, axis=1, kind="stable")
        top = order[:, :k]
        s_top = np.take_along_axis(sim, top, axis=1)
        gap = s_top[:, k - 1] - np.take_along_axis(sim, order[:, k:k + 1], axis=1)[:, 0] if k < feat.shape[0] else np.full(feat.shape[0], np.inf)
        w = s_top ** alpha
        info.append(dict(gap=gap, smin=s_top.min(axis=1), scale=(np.abs(w) * np.linalg.norm(feat, axis=1)[top]).sum(axis=1) / k))
        feat = (feat[top] * w[:, :, None]).mean(axis=1)
    if expand == "all":
        return feat[:q.shape[0]], feat[q.shape[0]:], info
    return q, feat, info


def inp_f64(distmat, qp, gp, qc, gc):
    """-> (mINP, inp float64 [nq], last_rank [nq] (0-based among the kept entries, -1 = invalid), n_rel [nq]).  Junk (same pid and same
    cam) is removed, the kept entries are ordered by (distance, gallery index); the mean runs over the queries with n_rel > 0."""
    distmat = np.asarray(distmat)
    qp, gp, qc, gc = (np.asarray(a) for a in (qp, gp, qc, gc))
    nq = distmat.shape[0]
    inp = np.zeros(nq, dtype=np.float64)
    last_rank = np.full(nq, -1, dtype=np.int64)
    n_rel = np.zeros(nq, dtype=np.int64)
    for i in range(nq):
        order = np.argsort(distmat[i], kind="stable")
        keep = ~((gp[order] == qp[i]) & (gc[order] == qc[i]))
        match = (gp[order] == qp[i])[keep]
        pos = np.nonzero(match)[0]
        n_rel[i] = pos.size
        if pos.size:
            last_rank[i] = pos[-1]
            inp[i] = pos.size / (pos[-1] + 1.0)
    valid = n_rel > 0
    return (float(inp[valid].mean()) if valid.any() else float("nan")), inp, last_rank, n_rel
