"""Writes tests/golden/roc.npz: sklearn.metrics.roc_curve (both drop settings) and roc_auc_score of pair ROC cases, small and medium
(a few thousand pairs each).  Needs scikit-learn (1.7.2 was used); the tests read the file and never import sklearn for it.
Run: python tests/golden/make_roc_golden.py"""
import os

import numpy as np

F32 = np.float32


def cases():
    """name -> (distmat fp32 [nq, ng], q_ids int32, g_ids int32)."""
    rng = np.random.default_rng(7)
    out = {}
    out["tiny_2x3"] = (np.array([[0.1, 0.5, 0.5], [0.9, 0.1, 0.5]], F32), np.array([0, 1], np.int32), np.array([0, 1, 1], np.int32))
    out["one_by_one"] = (np.array([[0.25]], F32), np.array([3], np.int32), np.array([3], np.int32))
    nq, ng = 23, 61
    out["random_23x61"] = (rng.uniform(0, 2, (nq, ng)).astype(F32), rng.integers(0, 6, nq).astype(np.int32), rng.integers(0, 6, ng).astype(np.int32))
    nq, ng = 40, 97
    out["levels_40x97"] = ((rng.integers(0, 16, (nq, ng)) / 8.0).astype(F32), rng.integers(0, 5, nq).astype(np.int32),
                           rng.integers(0, 5, ng).astype(np.int32))
    nq, ng = 31, 64
    out["binades_31x64"] = ((rng.choice([-1.0, 1.0], (nq, ng)) * np.exp2(rng.uniform(-30, 30, (nq, ng)))).astype(F32),
                            rng.integers(0, 4, nq).astype(np.int32), rng.integers(0, 4, ng).astype(np.int32))
    return out


def main():
    from sklearn.metrics import roc_auc_score, roc_curve
    z = {}
    for name, (d, qp, gp) in cases().items():
        y = np.int32(qp[:, None] == gp[None, :]).ravel()
        s = 1.0 - d.ravel() / 2.0
        assert s.dtype == F32
        z[name + "/distmat"], z[name + "/q_ids"], z[name + "/g_ids"] = d, qp, gp
        for drop in (True, False):
            fpr, tpr, thr = roc_curve(y, s, pos_label=1, drop_intermediate=drop)
            tag = "drop" if drop else "all"
            z["%s/fpr_%s" % (name, tag)], z["%s/tpr_%s" % (name, tag)], z["%s/thr_%s" % (name, tag)] = fpr, tpr, thr
        z[name + "/auc"] = np.float64(roc_auc_score(y, s))
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "roc.npz")
    np.savez_compressed(path, **z)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
