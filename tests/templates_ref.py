"""numpy restatements of the template kernels (include/daliid.h: dali_pool_rows, dali_segment_reduce2d, dali_open_set_search) and of
ops_eval.open_set_summary: float32 emulations that follow the documented arithmetic order operation by operation (every numpy float32
operation rounds once; a product is rounded before it is added: no FMA), float64 restatements to hold them against, and brute-force
versions of the open-set search (stable argsort) and summary (one probe at a time)."""
import numpy as np

F32 = np.float32


# ---- dali_pool_rows ----

def pool_f32(fvs, order, bounds, weights=None, mode="mean"):
    """Bit for bit what the kernel writes: one running sum per element over the members in member order."""
    fvs = np.ascontiguousarray(fvs, dtype=F32)
    T, d = len(bounds) - 1, fvs.shape[1]
    out = np.empty((T, d), dtype=F32)
    for t in range(T):
        rows = order[bounds[t]:bounds[t + 1]]
        if mode == "max":
            acc = np.full(d, -np.inf, dtype=F32)
            for r in rows:
                acc = np.where(fvs[r] > acc, fvs[r], acc)
            out[t] = acc
            continue
        acc, wsum = np.zeros(d, dtype=F32), F32(0)
        for r in rows:
            w = F32(1) if weights is None else F32(weights[r])
            acc = acc + (w * fvs[r]).astype(F32)
            wsum = F32(wsum + w)
        out[t] = acc / (F32(len(rows)) if weights is None else wsum)
    return out


def pool_f64(fvs, order, bounds, weights=None, mode="mean"):
    """-> (the pooled rows in float64, scale [T, d] = sum |w f| / sum w, counts [T]) from the same fp32 inputs."""
    f = np.asarray(fvs, dtype=np.float64)
    T, d = len(bounds) - 1, f.shape[1]
    out, scale = np.empty((T, d)), np.empty((T, d))
    for t in range(T):
        rows = order[bounds[t]:bounds[t + 1]]
        w = np.ones(len(rows)) if weights is None else np.asarray(weights, dtype=np.float64)[rows]
        if mode == "max":
            out[t], scale[t] = f[rows].max(axis=0), 0.0
        else:
            out[t] = (w[:, None] * f[rows]).sum(axis=0) / w.sum()
            scale[t] = (np.abs(w[:, None] * f[rows])).sum(axis=0) / w.sum()
    return out, scale, np.diff(np.asarray(bounds))


# ---- dali_segment_reduce2d ----

def _key(x):
    """the bit pattern as a signed integer that sorts like the value, -0.0 below +0.0"""
    k = np.ascontiguousarray(x, dtype=F32).view(np.int32)
    return k ^ ((k >> 31) & 0x7fffffff)


def _unkey(k):
    k = np.asarray(k, dtype=np.int32)
    return np.ascontiguousarray(k ^ ((k >> 31) & 0x7fffffff)).view(F32)


def segment_minmax(x, row_bounds, col_bounds, mode):
    """min / max of every block in the total order of the bit patterns: exact, whatever the order of the entries."""
    k = _key(x)
    red = np.minimum if mode == "min" else np.maximum
    rows = red.reduceat(k, np.asarray(row_bounds[:-1]), axis=0)
    return _unkey(red.reduceat(rows, np.asarray(col_bounds[:-1]), axis=1))


def segment_mean_f32(x, row_bounds, col_bounds):
    """Bit for bit: per column the running sum over the segment's rows (ascending), then the running sum of the column sums over the
    segment's columns (ascending), divided by float(|a| * |b|)."""
    x = np.ascontiguousarray(x, dtype=F32)
    Tr, Tc = len(row_bounds) - 1, len(col_bounds) - 1
    p = np.empty((Tr, x.shape[1]), dtype=F32)
    for a in range(Tr):
        acc = x[row_bounds[a]].copy()
        for r in range(row_bounds[a] + 1, row_bounds[a + 1]):
            acc = acc + x[r]
        p[a] = acc
    out = np.empty((Tr, Tc), dtype=F32)
    la = np.diff(np.asarray(row_bounds)).astype(np.int64)
    for b in range(Tc):
        acc = p[:, col_bounds[b]].copy()
        for j in range(col_bounds[b] + 1, col_bounds[b + 1]):
            acc = acc + p[:, j]
        out[:, b] = acc / (la * (col_bounds[b + 1] - col_bounds[b])).astype(F32)
    return out


def segment_mean_f64(x, row_bounds, col_bounds):
    """-> (block means in float64, block means of |x|) from the same fp32 entries."""
    x = np.asarray(x, dtype=np.float64)
    rb, cb = np.asarray(row_bounds), np.asarray(col_bounds)
    cnt = np.outer(np.diff(rb), np.diff(cb))
    s = np.add.reduceat(np.add.reduceat(x, rb[:-1], axis=0), cb[:-1], axis=1)
    sa = np.add.reduceat(np.add.reduceat(np.abs(x), rb[:-1], axis=0), cb[:-1], axis=1)
    return s / cnt, sa / cnt


# ---- dali_open_set_search / open_set_summary ----

def open_set_search(D, q_subj, g_subj):
    """Brute force, one probe at a time: the row sorted by a stable argsort, the other mates removed.
    -> (mate_dist f32, mate_col i32, nonmate_dist f32, nonmate_col i32, rank i32)"""
    D = np.asarray(D, dtype=F32)
    nq = D.shape[0]
    md, nd = np.full(nq, np.inf, dtype=F32), np.full(nq, np.inf, dtype=F32)
    mc, nc, rk = (np.full(nq, -1, dtype=np.int32) for _ in range(3))
    for i in range(nq):
        srt = np.argsort(D[i], kind="stable")
        mate = np.asarray(g_subj)[srt] == q_subj[i]
        if mate.any():
            best = srt[mate][0]
            md[i], mc[i] = D[i, best], best
            kept = srt[~mate | (srt == best)]              # the other mates removed
            rk[i] = int(np.nonzero(kept == best)[0][0])
        if (~mate).any():
            other = srt[~mate][0]
            nd[i], nc[i] = D[i, other], other
    return md, mc, nd, nc, rk


def open_set_summary(mate_dist, nonmate_dist, rank, fpirs, ranks):
    """The definition of ops_eval.open_set_summary restated probe by probe."""
    md, nd, rk = np.asarray(mate_dist, dtype=F32), np.asarray(nonmate_dist, dtype=F32), np.asarray(rank)
    mated = [i for i in range(len(rk)) if rk[i] >= 0]
    non = sorted(float(nd[i]) for i in range(len(rk)) if rk[i] < 0)
    nan = float("nan")
    res = dict(fnir={}, fpir={}, threshold={}, rank={}, n_mated=len(mated), n_nonmated=len(non))
    for r in ranks:
        res["rank"][r] = sum(1 for i in mated if rk[i] < r) / len(mated) if mated else nan
    for f in fpirs:
        m = int(np.floor(f * len(non) + 1e-9))
        thr = F32(non[m]) if m < len(non) else F32(np.inf)
        res["threshold"][f] = thr
        res["fpir"][f] = sum(1 for v in non if F32(v) < thr) / len(non) if non else nan
        for r in ranks:
            hit = sum(1 for i in mated if md[i] < thr and rk[i] < r)
            res["fnir"][(f, r)] = 1.0 - hit / len(mated) if mated else nan
    return res


def same_summary(a, b):
    """two summaries equal entry for entry (NaN equal to NaN)"""
    eq = lambda x, y: (np.isnan(x) and np.isnan(y)) or x == y
    if a["n_mated"] != b["n_mated"] or a["n_nonmated"] != b["n_nonmated"]:
        return False
    for name in ("fnir", "fpir", "threshold", "rank"):
        if set(a[name]) != set(b[name]) or not all(eq(a[name][k], b[name][k]) for k in a[name]):
            return False
    return True
