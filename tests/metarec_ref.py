"""numpy restatement of the meta-recognition contract of include/daliid.h (dali_mr_kill_transpose, dali_mr_fit_rows, dali_mr_wscore,
dali_mr_fuse), written from that contract: the reference of tests/test_gpu_metarec.py, pinned against the reference's own libmr /
Meta_Recognition in tests/test_metarec_cpu.py (tests/golden/metarec.npz).  Selections follow topk_ref.order."""
import numpy as np

from topk_ref import order

F32, F64 = np.float32, np.float64
ITERS, EPS = 100, 1e-6


def kill_transpose(S, topk, use_columns=False, killscale=1.0):
    """-> KT fp32 [ng, nq]: the topk largest entries of every row (use_columns: column) of S become fl32(s - fl32(killscale * s))."""
    KT = np.array(np.asarray(S, dtype=F32).T, dtype=F32, order="C", copy=True)       # KT[j][i] = S[i][j]
    ks = F32(killscale)
    if use_columns:
        for j in range(KT.shape[0]):
            o = order(KT[j], largest=True)[:topk]
            KT[j, o] = KT[j, o] - (ks * KT[j, o]).astype(F32)
    else:
        for i in range(KT.shape[1]):
            o = order(KT[:, i], largest=True)[:topk]
            KT[o, i] = KT[o, i] - (ks * KT[o, i]).astype(F32)
    return KT


def fit_row(row, T):
    """-> (shape, scale, small fp32, Newton steps).  Unfit: shape = scale = NaN."""
    row = np.asarray(row, dtype=F32)
    n = row.size
    o = order(row, largest=False)                  # ascending keys; the boundary key is the (n - T + 1)-th
    small = row[o[n - T]]
    v = row[o[n - T:]]                             # every key >= the boundary key: exactly T elements
    x = ((v + F32(1)).astype(F32) - small).astype(F32)
    with np.errstate(all="ignore"):
        L = np.log(x.astype(F64))
        l = L.astype(F32).astype(F64)
        mean_l = l.sum() / T
        k = 1.0
        for it in range(1, ITERS + 1):
            e = np.exp(k * L)
            fg, ff, ffp = e.sum(), (e * l).sum(), ((e * l) * l).sum()
            q = ff / fg
            f = q - mean_l - 1.0 / k
            fp = ffp / fg - q * q + 1.0 / (k * k)
            kn = k - f / fp
            if not (np.isfinite(f) and np.isfinite(fp) and np.isfinite(kn)):
                break
            if abs(kn - k) < EPS:
                return kn, (np.exp(kn * L).sum() / T) ** (1.0 / kn), small, it
            k = kn
    return np.nan, np.nan, small, it


def fit_rows(x, T):
    """-> (fits fp64 [nrows, 2], small fp32 [nrows], n_unfit, iters int32 [nrows])"""
    x = np.asarray(x, dtype=F32)
    fits, small, iters = np.empty((x.shape[0], 2), F64), np.empty(x.shape[0], F32), np.empty(x.shape[0], np.int32)
    for r in range(x.shape[0]):
        fits[r, 0], fits[r, 1], small[r], iters[r] = fit_row(x[r], T)
    return fits, small, int(np.isnan(fits[:, 0]).sum()), iters


def wscore(S, fits, small):
    S = np.asarray(S, dtype=F32)
    d = np.maximum(((S + F32(1)).astype(F32) - np.asarray(small, F32)[None, :]).astype(F32), F32(0))
    shape, scale = fits[:, 0][None, :], fits[:, 1][None, :]
    with np.errstate(all="ignore"):
        w = 1.0 - np.exp(-np.power(d.astype(F64) / scale, shape))
    unfit = np.isnan(shape) | np.isnan(scale)
    return np.where((d == 0) | unfit, 0.0, w)


def fuse_fitted(scores, fits, smalls):
    """-> (fused fp64, sum of w-scores fp64)"""
    num = den = tot = 0.0
    for S, f, sm in zip(scores, fits, smalls):
        s64 = np.asarray(S, dtype=F32).astype(F64)
        w = wscore(S, f, sm)
        num, den, tot = num + w * s64, den + w, tot + s64
    with np.errstate(all="ignore"):
        return np.where(den == 0, tot / len(scores), num / den), den


def metarec(S, topk, use_columns=True, killscale=1.0):
    """-> (fits, small, n_unfit) of the gallery columns of S [nq, ng]"""
    KT = kill_transpose(S, topk, use_columns, killscale)
    fits, small, n_unfit, _ = fit_rows(KT, KT.shape[1] - topk - 1)
    return fits, small, n_unfit


def mrfuse(scores, topk=20, use_columns=False, killscale=1.0):
    fitted = [metarec(S, topk, use_columns, killscale) for S in scores]
    return fuse_fitted(scores, [f[0] for f in fitted], [f[1] for f in fitted])
