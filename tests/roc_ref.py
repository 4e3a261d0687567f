"""numpy restatement of the pair ROC as include/daliid.h (dali_roc_build) defines it, and of the verification summary
(ops_eval.verification_summary); test infrastructure only.  The curve is formed the way sklearn 1.7.2 forms it (stable mergesort,
distinct values by np.diff, float64 counts), so its output is bitwise sklearn's without importing it."""
import warnings

import numpy as np

F32 = np.float32


class UndefinedMetricWarning(UserWarning):
    pass


def pair_scores_labels(distmat, q_ids, g_ids):
    """score fl32(1 - fl32(d / 2)) and label q_id == g_id of every pair, row-major."""
    d = np.asarray(distmat, dtype=F32)
    s = (F32(1.0) - d / F32(2.0)).astype(F32).ravel()
    y = (np.asarray(q_ids)[:, None] == np.asarray(g_ids)[None, :]).ravel()
    return s, y


def counts(scores, labels):
    """-> (fps, tps, thresholds) at every distinct score, descending (sklearn's _binary_clf_curve)."""
    s = np.asarray(scores, dtype=F32)
    if not np.all(np.isfinite(s)):
        raise ValueError("Input contains NaN or infinity.")
    y = np.asarray(labels).astype(bool)
    order = np.argsort(s, kind="mergesort")[::-1]
    s, y = s[order], y[order]
    idx = np.r_[np.nonzero(np.diff(s))[0], y.size - 1]
    tps = np.cumsum(y, dtype=np.float64)[idx]
    fps = 1 + idx - tps
    return fps, tps, s[idx]


def curve_from_counts(fps, tps, thr, drop_intermediate=True):
    if drop_intermediate and len(fps) > 2:
        keep = np.nonzero(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]
        fps, tps, thr = fps[keep], tps[keep], thr[keep]
    fps, tps = np.r_[0, fps], np.r_[0, tps]
    thr = np.r_[np.inf, thr]
    if fps[-1] <= 0:
        warnings.warn("No negative samples in y_true, false positive value should be meaningless", UndefinedMetricWarning)
        fpr = np.repeat(np.nan, fps.shape)
    else:
        fpr = fps / fps[-1]
    if tps[-1] <= 0:
        warnings.warn("No positive samples in y_true, true positive value should be meaningless", UndefinedMetricWarning)
        tpr = np.repeat(np.nan, tps.shape)
    else:
        tpr = tps / tps[-1]
    return fpr, tpr, thr


def roc_curve_scores(scores, labels, drop_intermediate=True):
    return curve_from_counts(*counts(scores, labels), drop_intermediate=drop_intermediate)


def roc_curve(distmat, q_ids, g_ids, drop_intermediate=True):
    return roc_curve_scores(*pair_scores_labels(distmat, q_ids, g_ids), drop_intermediate=drop_intermediate)


def verification_metrics(distmat, q_ids, g_ids, fars=(1e-1, 1e-2, 1e-3, 1e-4, 1e-5, 1e-6)):
    s, y = pair_scores_labels(distmat, q_ids, g_ids)
    fps, tps, thr = counts(s, y)
    fpr, tpr, t = curve_from_counts(fps, tps, thr, True)
    fa, ta, tha = curve_from_counts(fps, tps, thr, False)
    auc = float(np.trapezoid(tpr, fpr))
    eer = eer_thr = float("nan")
    for k in range(len(fpr)):
        if fpr[k] + tpr[k] >= 1.0:
            if k == 0:
                eer, eer_thr = float(fpr[0]), float(t[0])
            else:
                f0, t0, f1, t1 = fpr[k - 1], tpr[k - 1], fpr[k], tpr[k]
                lam = (1.0 - t0 - f0) / ((f1 - f0) + (t1 - t0))
                eer, eer_thr = float(f0 + lam * (f1 - f0)), float(t[k])
            break
    tar = {}
    for f in fars:
        best, bthr = float("nan"), float("nan")
        for k in range(len(fa)):                       # points in curve order: tpr never decreases
            if fa[k] <= f and (best != best or ta[k] > best):
                best, bthr = float(ta[k]), float(tha[k])
        tar[f] = (best, bthr)
    return dict(n_pos=int(y.sum()), n_neg=int(y.size - y.sum()), auc=auc, eer=eer, eer_threshold=eer_thr, tar_at_far=tar)
