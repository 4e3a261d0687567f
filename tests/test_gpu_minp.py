"""GPU: mINP (ops_eval.rank_eval_inp, dali_rank_eval_inp) against tests/qe_ref.inp_f64: last_rank and n_rel exactly, inp bit for bit the
fp32 quotient, mINP within 1e-12 relative of the float64 mean; and rank_eval's outputs unchanged around it."""
import contextlib
import io

import numpy as np
import pytest
import torch

import qe_ref as R

pytestmark = pytest.mark.gpu

F32 = np.float32
RANK_PSMALL = 512          # csrc/rank.hip: more same-identity gallery entries than this send a query to the second launch


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    torch.cuda.set_device(0)
    return torch.device("cuda", 0)


def _random(seed, nq, ng, n_ids=5, n_cams=3, ties=False):
    rng = np.random.default_rng(seed)
    d = rng.uniform(0, 2, (nq, ng)).astype(F32)
    if ties:
        d = (np.round(d * 8) / 8).astype(F32)
    return d, rng.integers(0, n_ids, nq), rng.integers(0, n_ids, ng), rng.integers(0, n_cams, nq), rng.integers(0, n_cams, ng)


def _synthetic():
    from oracle import evalrank as E
    q, g, qp, gp, qc, gc = E.synthetic_reid_set(20, 10, 2, 256, noise=2.4, seed=1)
    return E.validate_features(q, g).numpy().astype(F32), qp, gp, qc, gc


def _invalid_queries():
    """query 2: its identity is not in the gallery; query 3: its identity only at its own camera (junk).  Both are left out."""
    d, qp, gp, qc, gc = _random(21, 6, 64)
    qp[2] = 99
    qp[3], qc[3] = 7, 1
    gp[5], gc[5], gp[40], gc[40] = 7, 1, 7, 1
    return d, qp, gp, qc, gc


def _large_identity():
    """identity 0 has 600 gallery entries (> RANK_PSMALL): its queries are redone by the second launch; identity 1 stays in the first"""
    d, qp, gp, qc, gc = _random(22, 7, 700, n_ids=2)
    gp[:600], gp[600:] = 0, 1
    qp[:] = [0, 1, 0, 1, 0, 1, 0]
    assert (gp == 0).sum() > RANK_PSMALL
    return d, qp, gp, qc, gc


def _all_at_position_one():
    """every query has exactly one match, at distance 0 with everything else farther: INP = 1 for all, mINP = 1.0 exactly"""
    rng = np.random.default_rng(23)
    nq, ng = 8, 40
    d = rng.uniform(0.5, 2, (nq, ng)).astype(F32)
    qp, gp = np.arange(nq), np.full(ng, 100)
    qc, gc = np.zeros(nq, dtype=np.int64), np.ones(ng, dtype=np.int64)
    for i in range(nq):
        gp[3 * i + 1] = i
        d[i, 3 * i + 1] = 0.0
    return d, qp, gp, qc, gc


CASES = {
    "synthetic": _synthetic,
    "ng37_scalar": lambda: _random(1, 9, 37),
    "ng64": lambda: _random(2, 9, 64),
    "ng4100_vector_and_tail": lambda: _random(3, 9, 4100),
    "ties_ng64": lambda: _random(4, 9, 64, ties=True),
    "ties_ng203": lambda: _random(5, 9, 203, ties=True),
    "invalid_queries": _invalid_queries,
    "large_identity": _large_identity,
    "all_at_position_one": _all_at_position_one,
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_rank_eval_inp(dev, name):
    from daliid_amd import ops_eval
    d, qp, gp, qc, gc = CASES[name]()
    want_minp, want_inp, want_last, want_nrel = R.inp_f64(d, qp, gp, qc, gc)
    dd = torch.from_numpy(d).to(dev)
    before = ops_eval.rank_eval(dd, qp, gp, qc, gc, return_per_query=True)
    minp, inp, last_rank, n_rel = ops_eval.rank_eval_inp(dd, qp, gp, qc, gc, return_per_query=True)
    after = ops_eval.rank_eval(dd, qp, gp, qc, gc, return_per_query=True)
    assert last_rank.dtype == np.int32 and n_rel.dtype == np.int32 and inp.dtype == F32
    assert np.array_equal(last_rank, want_last) and np.array_equal(n_rel, want_nrel)
    valid = want_nrel > 0
    quotient = np.where(valid, want_nrel.astype(F32) / np.maximum(want_last + 1, 1).astype(F32), F32(0)).astype(F32)
    assert np.array_equal(inp.view(np.uint32), quotient.view(np.uint32))
    assert abs(minp - want_minp) <= 1e-12 * abs(want_minp), (minp, want_minp)
    assert ops_eval.rank_eval_inp(dd, qp, gp, qc, gc) == minp
    # rank_eval around the call: bit for bit itself
    assert np.array_equal(before[0].view(np.uint32), after[0].view(np.uint32)) and before[1] == after[1]
    assert np.array_equal(before[2].view(np.uint32), after[2].view(np.uint32)) and np.array_equal(before[3], after[3])
    # the two entries agree on what a valid query is and on where its first match is
    assert np.array_equal(before[3] >= 0, valid) and np.all(before[3][valid] <= last_rank[valid])
    if name == "invalid_queries":
        assert last_rank[2] == -1 and last_rank[3] == -1 and n_rel[2] == 0 and n_rel[3] == 0 and valid.sum() == 4
    if name == "all_at_position_one":
        assert minp == 1.0 and np.all(inp == 1.0)
    if name == "large_identity":
        assert n_rel[0] > RANK_PSMALL // 2 and valid.all()


def test_rank_eval_inp_raises_what_rank_eval_raises(dev):
    from daliid_amd import _lib, ops_eval
    d, qp, gp, qc, gc = _random(31, 4, 64)
    dd = torch.from_numpy(d).to(dev)
    with pytest.raises(AssertionError, match="do not appear in gallery"):
        ops_eval.rank_eval_inp(dd, qp + 50, gp, qc, gc)
    d, qp, gp, qc, gc = _random(32, 2, 4200, n_ids=1)           # 4200 > 4096 entries of one identity: the documented limit
    with pytest.raises(_lib.DaliError, match="4096"):
        ops_eval.rank_eval_inp(torch.from_numpy(d).to(dev), qp, gp, qc, gc)


def test_validator_reports_minp(dev):
    from daliid_amd import ops_eval, validateModels as V
    d, qp, gp, qc, gc = _synthetic()
    queries = np.stack([np.arange(qp.size), qp, qc], axis=1)
    gallery = np.stack([np.arange(gp.size), gp, gc], axis=1)
    dd = torch.from_numpy(d).to(dev)
    v = V.validationManager.getValidator("Market")
    v.setParameters(64, 32, False, 0)
    assert v.report_minp is False and not hasattr(v, "mINP")
    plain_out = io.StringIO()
    with contextlib.redirect_stdout(plain_out):
        cmc0, map0 = v.calculateMetrics(dd, queries, gallery)
    assert "mINP" not in plain_out.getvalue() and not hasattr(v, "mINP")
    v.report_minp = True
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        cmc1, map1 = v.calculateMetrics(dd, queries, gallery)
    assert v.mINP == ops_eval.rank_eval_inp(dd, qp, gp, qc, gc)
    assert map1 == map0 and np.array_equal(cmc1.view(np.uint32), cmc0.view(np.uint32))
    assert "mINP: {:.2%}".format(v.mINP) in out.getvalue()
    assert out.getvalue().replace("mINP: {:.2%}\n".format(v.mINP), "") == plain_out.getvalue()
