"""CPU: the numpy restatement of the pair ROC (tests/roc_ref.py) against sklearn 1.7.2's recorded outputs (tests/golden/roc.npz) bit for
bit, against sklearn itself on random cases when it is installed, and on hand-worked cases of the definition's corner rules."""
import warnings

import numpy as np
import pytest

import roc_ref as R
from conftest import load_golden

F32 = np.float32


def _names(z):
    return sorted({k.split("/")[0] for k in z.files})


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (a, b)


@pytest.fixture(scope="module")
def golden():
    return load_golden("roc.npz")


def test_reference_matches_sklearn_goldens_bitwise(golden):
    z = golden
    for name in _names(z):
        d, qp, gp = z[name + "/distmat"], z[name + "/q_ids"], z[name + "/g_ids"]
        for drop, tag in ((True, "drop"), (False, "all")):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                fpr, tpr, thr = R.roc_curve(d, qp, gp, drop_intermediate=drop)
            _same(fpr, z["%s/fpr_%s" % (name, tag)])
            _same(tpr, z["%s/tpr_%s" % (name, tag)])
            _same(thr, z["%s/thr_%s" % (name, tag)])
        auc = z[name + "/auc"]
        if np.isfinite(auc):
            assert R.verification_metrics(d, qp, gp)["auc"] == float(auc), name


def test_reference_matches_sklearn_random():
    metrics = pytest.importorskip("sklearn.metrics")
    rng = np.random.default_rng(3)
    for trial in range(12):
        nq, ng = rng.integers(1, 40, 2)
        d = rng.uniform(0, 2, (nq, ng)).astype(F32)
        if trial % 3 == 0:
            d = (np.round(d * 4) / 4).astype(F32)
        qp, gp = rng.integers(0, 4, nq), rng.integers(0, 4, ng)
        y = (qp[:, None] == gp[None, :]).ravel().astype(np.int32)
        s = 1.0 - d.ravel() / 2.0
        for drop in (True, False):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                want = metrics.roc_curve(y, s, pos_label=1, drop_intermediate=drop)
                got = R.roc_curve(d, qp, gp, drop_intermediate=drop)
            for a, b in zip(got, want):
                _same(a, b)
        if 0 < y.sum() < y.size:
            assert R.verification_metrics(d, qp, gp)["auc"] == metrics.roc_auc_score(y, s)


def test_positive_and_negative_tied_at_one_score():
    fpr, tpr, thr = R.roc_curve(np.array([[0.5, 0.5]], F32), [1], [1, 2])
    _same(thr, np.array([np.inf, 0.75], F32))
    _same(fpr, np.array([0.0, 1.0]))
    _same(tpr, np.array([0.0, 1.0]))


def test_all_scores_equal_is_two_points():
    d = np.full((5, 7), 0.3, F32)
    fpr, tpr, thr = R.roc_curve(d, np.arange(5) % 3, np.arange(7) % 3)
    assert len(thr) == 2 and thr[1] == F32(1) - F32(0.3) / F32(2)


def test_one_by_one():
    fpr, tpr, thr = R.roc_curve(np.array([[1.0]], F32), [0], [1])
    _same(thr, np.array([np.inf, 0.5], F32))


def test_equal_step_diagonal_runs_drop_and_unequal_steps_stay():
    # four distinct scores, each one positive and one negative: equal steps, the interior points go
    d = np.array([[0.0, 0.2, 0.4, 0.6], [0.0, 0.2, 0.4, 0.6]], F32)
    fpr, tpr, thr = R.roc_curve(d, [0, 1], [0, 0, 0, 0])
    assert len(thr) == 3
    _same(fpr, np.array([0.0, 0.25, 1.0]))
    fa, ta, _ = R.roc_curve(d, [0, 1], [0, 0, 0, 0], drop_intermediate=False)
    assert len(fa) == 5
    # unequal steps on one line (1 then 2 negatives per score) are kept
    d2 = np.array([[0.0, 0.2, 0.2, 0.4]], F32)
    f2, t2, th2 = R.roc_curve(d2, [9], [0, 1, 2, 3])
    assert len(th2) == 4


def test_tar_uses_the_undropped_curve():
    d = np.array([[0.0, 0.2, 0.4, 0.6], [0.0, 0.2, 0.4, 0.6]], F32)
    m = R.verification_metrics(d, [0, 1], [0, 0, 0, 0], fars=(0.5,))
    assert m["tar_at_far"][0.5][0] == 0.5


def test_no_positives_warns_and_gives_nan():
    with pytest.warns(UserWarning):
        fpr, tpr, thr = R.roc_curve(np.array([[0.1, 0.2]], F32), [0], [1, 2])
    assert np.isnan(tpr).all() and not np.isnan(fpr).any()


def test_nan_input_raises():
    with pytest.raises(ValueError):
        R.roc_curve(np.array([[0.1, np.nan]], F32), [0], [0, 1])
