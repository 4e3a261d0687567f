"""CPU: the host side of template evaluation -- ops_eval.template_index, ops_eval.open_set_summary against a probe-by-probe
restatement, the argument refusals of validateModels.setTemplates, and the numpy emulations of tests/templates_ref.py (what the GPU
tests hold the kernels against, bit for bit) against their own float64 restatements."""
import numpy as np
import pytest

import templates_ref as R

F32 = np.float32


# ---- template_index ----

def _check_index(keys_rows, order, bounds, first):
    """first-appearance numbering, stable member order, every row once"""
    n = len(keys_rows)
    assert order.dtype == np.int32 and bounds.dtype == np.int32 and first.dtype == np.int64
    assert sorted(order.tolist()) == list(range(n)) and bounds[0] == 0 and bounds[-1] == n and np.all(np.diff(bounds) > 0)
    seen = []
    for k in keys_rows:
        if k not in seen:
            seen.append(k)
    assert len(seen) == len(bounds) - 1 == len(first)
    for t, k in enumerate(seen):
        members = order[bounds[t]:bounds[t + 1]].tolist()
        assert members == [i for i in range(n) if keys_rows[i] == k]
        assert first[t] == members[0]


def test_template_index_string_keys():
    from daliid_amd import ops_eval
    keys = np.array(["trk_b", "trk_a", "trk_b", "zz", "trk_a", "trk_b", "a"])
    _check_index(keys.tolist(), *ops_eval.template_index(keys))


def test_template_index_tuple_keys():
    from daliid_amd import ops_eval
    rng = np.random.default_rng(0)
    pid, cam = rng.integers(0, 5, 200), rng.integers(0, 3, 200).astype(str)
    order, bounds, first = ops_eval.template_index((pid, cam))
    _check_index(list(zip(pid.tolist(), cam.tolist())), order, bounds, first)
    three = ops_eval.template_index((pid, cam, np.zeros(200)))
    assert all(np.array_equal(a, b) for a, b in zip(three, (order, bounds, first)))


def test_template_index_one_template_and_singletons():
    from daliid_amd import ops_eval
    order, bounds, first = ops_eval.template_index(np.full(9, 4))
    assert order.tolist() == list(range(9)) and bounds.tolist() == [0, 9] and first.tolist() == [0]
    order, bounds, first = ops_eval.template_index(np.array([5, 3, 9, 1, 7]))
    assert order.tolist() == list(range(5)) and bounds.tolist() == list(range(6)) and first.tolist() == list(range(5))
    order, bounds, first = ops_eval.template_index(np.zeros(0))
    assert order.size == 0 and bounds.tolist() == [0] and first.size == 0


def test_template_index_refusals():
    from daliid_amd import ops_eval
    with pytest.raises(ValueError):
        ops_eval.template_index((np.arange(4), np.arange(5)))
    with pytest.raises(ValueError):
        ops_eval.template_index(np.zeros((3, 2)))
    with pytest.raises(ValueError):
        ops_eval.template_index(())


# ---- open_set_summary ----

FPIRS, RANKS = (1e-1, 1e-2, 1e-3), (1, 20)


def _probes(rng, n_mated, n_non, levels):
    """integer-valued distances from few levels: ties among the non-mated probes and between mate distances and the thresholds"""
    n = n_mated + n_non
    rank = np.concatenate([rng.integers(0, 40, n_mated), np.full(n_non, -1)]).astype(np.int32)
    mate = np.concatenate([rng.integers(0, levels, n_mated), np.full(n_non, np.inf)]).astype(F32)
    non = rng.integers(0, levels, n).astype(F32)
    p = rng.permutation(n)
    return mate[p], non[p], rank[p]


@pytest.mark.parametrize("n_mated,n_non,levels", [(50, 10, 6), (120, 300, 9), (400, 3000, 50), (7, 1, 3), (33, 47, 1000), (60, 0, 6), (0, 25, 6)])
def test_open_set_summary_against_brute_force(n_mated, n_non, levels):
    """10, 300 and 3000 non-mated probes put fpir * N_nm on an integer (0.1 x 10 = 1, 0.01 x 300 = 3, 0.001 x 3000 = 3); the last two
    cases have no non-mated / no mated probes"""
    from daliid_amd import ops_eval
    rng = np.random.default_rng(n_mated * 31 + n_non)
    mate, non, rank = _probes(rng, n_mated, n_non, levels)
    got = ops_eval.open_set_summary(mate, non, rank, FPIRS, RANKS)
    want = R.open_set_summary(mate, non, rank, FPIRS, RANKS)
    assert R.same_summary(got, want), (got, want)
    assert got["n_mated"] == n_mated and got["n_nonmated"] == n_non
    for f in FPIRS:
        if n_non:
            assert got["fpir"][f] <= f + 1e-12          # strict acceptance below the (m + 1)-th smallest: never more than m false alarms
        else:
            assert got["threshold"][f] == np.inf and np.isnan(got["fpir"][f])
        for r in RANKS:
            assert np.isnan(got["fnir"][(f, r)]) if n_mated == 0 else 0.0 <= got["fnir"][(f, r)] <= 1.0


def test_open_set_summary_by_hand():
    """10 non-mated probes with nonmate_dist 0 .. 9: fpir 0.1 -> m = 1, T = 1, one false alarm (the 0); a mate at exactly T is rejected"""
    from daliid_amd import ops_eval
    non = np.concatenate([np.arange(10), np.full(4, 9.0)]).astype(F32)
    mate = np.concatenate([np.full(10, np.inf), [0.5, 1.0, 0.5, 0.0]]).astype(F32)
    rank = np.concatenate([np.full(10, -1), [0, 0, 3, 25]]).astype(np.int32)
    s = ops_eval.open_set_summary(mate, non, rank, fpirs=(0.1, 0.5), ranks=(1, 20))
    assert s["threshold"][0.1] == 1.0 and s["fpir"][0.1] == 0.1
    assert s["fnir"][(0.1, 1)] == 0.75 and s["fnir"][(0.1, 20)] == 0.5           # rank 1: only the first; rank 20: first and third
    assert s["threshold"][0.5] == 5.0 and s["fpir"][0.5] == 0.5
    assert s["fnir"][(0.5, 1)] == 0.5 and s["fnir"][(0.5, 20)] == 0.25 and s["rank"] == {1: 0.5, 20: 0.75}
    # exact ties at the threshold among the non-mated probes: nothing at the threshold is accepted, the realised FPIR falls below fpir
    tied = ops_eval.open_set_summary(np.full(10, np.inf, dtype=F32), np.full(10, 3.0, dtype=F32), np.full(10, -1), fpirs=(0.5,), ranks=(1,))
    assert tied["threshold"][0.5] == 3.0 and tied["fpir"][0.5] == 0.0 and np.isnan(tied["fnir"][(0.5, 1)])
    with pytest.raises(ValueError):
        ops_eval.open_set_summary(mate, non[:5], rank)


# ---- setTemplates ----

def test_set_templates_refusals_and_switch():
    from daliid_amd import validateModels as V
    for v in (V.validationManager.getValidator("Market"), V.validationManager.getValidator("BRIAR")):
        assert v.templates is None and v.report_open_set is False
        for kwargs in (dict(query=1, pooling="median"), dict(query=1, linkage="average"), dict(query=1.5), dict(gallery="pid"),
                       dict(query=(1, "cam")), dict(query=()), dict(gallery=-1), dict(query=True)):
            with pytest.raises(ValueError):
                v.setTemplates(**kwargs)
            assert v.templates is None
        v.setTemplates(query=(1, 2), gallery=lambda subset: subset[:, 1], pooling="unit_mean")
        assert v.templates["query"] == (1, 2) and v.templates["pooling"] == "unit_mean" and v.templates["linkage"] is None
        v.setTemplates(query=1, linkage="min")
        assert v.templates["linkage"] == "min" and v.templates["gallery"] is None
        v.setQueryExpansion(k=5)
        with pytest.raises(ValueError, match="query expansion"):
            v.validate(None, None, None)                   # refused before the model or a feature is touched
        v.setQueryExpansion(None)
        with pytest.raises(NotImplementedError, match="linkage"):
            v.retrieve(None, None, None)
        with pytest.raises(NotImplementedError, match="template"):
            v.validate_sharded(None, None, None)
        v.setTemplates()
        assert v.templates is None and v.template_rows is None


def test_template_rows_and_mixed_cameras():
    """one row per template (its first member's); a template whose members' cameras disagree gets a camera id that equals no camera of
    either side, also in a fixed-width string column, which must not truncate it"""
    from daliid_amd import validateModels as V
    v = V.validationManager.getValidator("Market")
    q = np.array([["a.jpg", "7", "c1"], ["b.jpg", "7", "c2"], ["c.jpg", "8", "c1"], ["d.jpg", "8", "c1"], ["e.jpg", "9", "c3"]])
    g = np.array([["f.jpg", "7", "c1"], ["g.jpg", "7", "c1"], ["h.jpg", "9", "c2"], ["i.jpg", "9", "c3"]])
    v.setTemplates(query=1, gallery=1)
    sides, (qr, gr) = v._template_sides(q, g)
    assert qr[:, 0].tolist() == ["a.jpg", "c.jpg", "e.jpg"] and qr[:, 1].tolist() == ["7", "8", "9"]
    assert gr[:, 0].tolist() == ["f.jpg", "h.jpg"]
    cams = set(q[:, 2]) | set(g[:, 2])
    assert qr[0, 2] not in cams and gr[1, 2] not in cams and qr[0, 2] != gr[1, 2] and len(qr[0, 2]) > 2
    assert qr[1:, 2].tolist() == ["c1", "c3"] and gr[0, 2] == "c1"
    assert sides[0][0].tolist() == [0, 1, 2, 3, 4] and sides[0][1].tolist() == [0, 2, 4, 5]
    qi = np.array([[0, 7, 1], [1, 7, 2], [2, 8, 1]], dtype=np.int32)
    gi = np.array([[3, 7, 1], [4, 8, 5], [5, 8, 6]], dtype=np.int32)
    _, (qr, gr) = v._template_sides(qi, gi)
    assert qr[0, 2] not in (1, 2, 5, 6) and gr[1, 2] not in (1, 2, 5, 6) and qr[0, 2] != gr[1, 2] and qr[1, 2] == 1 and gr[0, 2] == 1
    v.setTemplates(query=(1, 2))                                  # multi-query by pid and camera: no template mixes cameras
    sides, (qr, gr) = v._template_sides(q, g)
    assert sides[1] is None and gr is g and qr[:, 2].tolist() == ["c1", "c2", "c1", "c3"]


# ---- the emulations against their float64 restatements ----

def _templates(rng, lengths, n_extra=0):
    n = int(sum(lengths)) + n_extra
    bounds = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
    order = rng.permutation(n)[:bounds[-1]].astype(np.int32)
    return n, order, bounds


@pytest.mark.parametrize("weighted", [False, True])
def test_pool_emulation_against_float64(weighted):
    """per element |emulation - float64| <= (n_t + 3) 2^-24 sum |w f| / sum w: n_t products, n_t additions of which the first is exact,
    the division, and the weight sum's own n_t - 1 roundings (relative, first order; the same bound for any summation order)"""
    rng = np.random.default_rng(5)
    lengths = [1, 2, 63, 64, 65, 300]
    n, order, bounds = _templates(rng, lengths, n_extra=7)
    fvs = (rng.standard_normal((n, 37)) * rng.uniform(0.5, 2, (n, 1))).astype(F32)
    w = rng.uniform(0.25, 4, n).astype(F32) if weighted else None
    got = R.pool_f32(fvs, order, bounds, w).astype(np.float64)
    ref, scale, counts = R.pool_f64(fvs, order, bounds, w)
    assert np.all(np.abs(got - ref) <= (counts[:, None] + 3) * 2.0 ** -24 * scale)
    assert np.array_equal(R.pool_f32(fvs, order, bounds, mode="max"), R.pool_f64(fvs, order, bounds, mode="max")[0].astype(F32))
    one = R.pool_f32(fvs, np.arange(n, dtype=np.int32), np.arange(n + 1, dtype=np.int32))
    assert np.array_equal(one, fvs)                               # singletons without weights: (0 + 1 f) / 1


def test_segment_emulations_against_float64():
    rng = np.random.default_rng(6)
    rb = np.concatenate([[0], np.cumsum([1, 2, 64, 65, 30])])
    cb = np.concatenate([[0], np.cumsum([65, 1, 2, 40, 64])])
    x = rng.integers(-3, 4, (rb[-1], cb[-1])).astype(F32)
    x[x == 0] = np.where(rng.random(np.count_nonzero(x == 0)) < 0.5, F32(-0.0), F32(0.0))
    x[0, 0], x[5, 70] = np.inf, np.inf
    for mode, red in (("min", np.min), ("max", np.max)):
        got = R.segment_minmax(x, rb, cb, mode)
        for a in range(len(rb) - 1):
            for b in range(len(cb) - 1):
                blk = x[rb[a]:rb[a + 1], cb[b]:cb[b + 1]]
                assert got[a, b] == red(blk)
                if got[a, b] == 0:                                # -0.0 sorts below +0.0, whatever the order of the entries
                    has_neg, has_pos = np.any(np.signbit(blk[blk == 0])), np.any(~np.signbit(blk[blk == 0]))
                    assert np.signbit(got[a, b]) == (has_neg if mode == "min" else not has_pos)
    y = rng.standard_normal(x.shape).astype(F32)
    got = R.segment_mean_f32(y, rb, cb).astype(np.float64)
    ref, mean_abs = R.segment_mean_f64(y, rb, cb)
    cnt = np.outer(np.diff(rb), np.diff(cb))
    assert np.all(np.abs(got - ref) <= (cnt + 1) * 2.0 ** -24 * mean_abs)
    xi = np.abs(np.where(np.isinf(x), F32(1), x))                 # small integers: every sum exact, one rounding in the division
    ints, ref = R.segment_mean_f32(xi, rb, cb), R.segment_mean_f64(xi, rb, cb)[0]
    assert np.array_equal(ints, ref.astype(F32))


def test_open_set_search_restatement_by_hand():
    D = np.array([[3, 1, 1, 2, 1], [5, 5, 5, 5, 5], [0, 2, 2, 9, 9]], dtype=F32)
    g = np.array([4, 7, 4, 4, 8])
    md, mc, nd, nc, rk = R.open_set_search(D, np.array([4, 9, 8]), g)
    assert md.tolist() == [1, np.inf, 9] and mc.tolist() == [2, -1, 4]
    assert nd.tolist() == [1, 5, 0] and nc.tolist() == [1, 0, 0]
    assert rk.tolist() == [1, -1, 4]            # probe 0: column 1 ties the best mate and comes first; column 4 ties and comes after
